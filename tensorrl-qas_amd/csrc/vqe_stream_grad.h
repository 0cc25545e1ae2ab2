// vqe_stream_grad.h - adjoint energy gradient of the HBM-streaming path (n >= 14), DESIGN 4.9.
//
// The algorithm of vqe_grad.h for states that live in HBM:
//  1. forward: stream_evaluate without the energy leaves psi of every stream in the physical frame of its GF(2) map
//     (sw.states) together with the compiled ops, the frame (sw.masks, sw.meta) and (cos, sin) of the angles (sw.cs);
//     k_s_terms moves the Pauli masks of this handle's shard into that frame;
//  2. k_sg_lambda: lambda = H_shard psi in the physical frame - a thread owns amplitudes, not pairs, so no two threads
//     write one lambda entry - and E = Re <psi|lambda>, block partials reduced by k_s_reduce;
//  3. k_sg_back<K>: for the op groups of k_s_opk in reverse, K ops per read-modify-write sweep over psi AND lambda
//     (64 * 2^n bytes per sweep): for op j = last .. first of the group the contribution Re <lambda| K_j psi> (K_j the op
//     at (cos, sin) = (0, 1)) is block-summed into gpart[b][op][block], then U_j^-1 = U_j(cos, -sin) is applied to both;
//  4. k_sg_reduce: grad[j] = sum over the ops with parameter j, each summed over its blocks, in one fixed order
//     (bitwise reproducible, no atomics; exactly 0 for a parameter no op uses).
// After a gradient sw.states holds the INITIAL state again (every op undone) and sw.lam the pulled-back lambda.
// The noiseless instances see rotations only (noise without vqe_set_stream_noise_grad is refused before this path is
// entered, vqe_api.hip: grad_refusal) and skip an op of any other kind.
// NOISY (vqe_set_stream_noise_grad): the mean over T frozen Pauli-noise realisations.  The B * T (circuit,
// realisation) pairs are virtual streams of an expanded batch (k_sn_expand: the gates of circuit b, a theta slot and a
// gradient row of their own, the draw key (b, eval_base + t)), `resident` of them per chunk through the same launches;
// the backward sweep is the <K, PZ = true> instance, which applies the OP_PZ records of the drawn Z / Y errors to psi and
// lambda (a +-1 diagonal: its own inverse, no gradient row); k_sg_mean closes the run after the last chunk.
#pragma once
#include "vqe_stream.h"
#include "noise_grad_host.h"

namespace vqe {

constexpr int kGradOpsPerSweep = 3;   // K of k_sg_back: the largest that compiles for gfx950 without scratch
constexpr int kLambdaApt = 2;         // amplitudes a thread of k_sg_lambda owns

// s_apply_k with the angle given as (cos, sin) instead of read from the parameter table, and with the dependent-mask
// case spelled out per flip code (static register indices only: no scratch).  Ops that are no rotation are skipped;
// PZ: the record of a drawn Z error, (-1)^(parity(idx & zm) ^ inv), is applied (OP_NOP stays skipped).
template <int K, bool PZ = false>
__device__ __forceinline__ void s_apply_k_cs(double2 (&v)[1 << K], const uint32_t (&idx)[1 << K], const Op op,
                                             const double2 c, const int flip) {
  constexpr int E = 1 << K;
  const int kind = op.kind & 0xff, inv = (op.kind >> 8) & 1;
  if (op_is_pair(kind)) {
    if (flip < 1 || flip >= E) return;
    double2 w[E];
#pragma unroll
    for (int f = 1; f < E; ++f)      // own slot (f a power of two) or a combination of the slots (dependent mask)
      if (flip == f) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double2 a = v[e], bq = v[e ^ f];
          if (kind == OP_RX) w[e] = make_double2(c.x * a.x - c.y * bq.y, c.x * a.y + c.y * bq.x);
          else if (kind == OP_RY) {
            const double sg = (parity32(idx[e] & op.zm) ^ inv) ? -c.y : c.y;
            w[e] = make_double2(c.x * a.x + sg * bq.x, c.x * a.y + sg * bq.y);
          } else {
            const double sg = (parity32(idx[e] & op.zm) ^ inv) ? c.y : -c.y;
            w[e] = make_double2(c.x * a.x - sg * bq.y, c.x * a.y + sg * bq.x);
          }
        }
      }
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = w[e];
  } else if (kind == OP_RZ) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double sg = (parity32(idx[e] & op.zm) ^ inv) ? -c.y : c.y;
      const double2 a = v[e];
      v[e] = make_double2(c.x * a.x - sg * a.y, c.x * a.y + sg * a.x);
    }
  } else if (PZ && kind == OP_PZ) {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (parity32(idx[e] & op.zm) ^ inv) v[e] = make_double2(-v[e].x, -v[e].y);
  }
}

// lambda = H_shard psi (physical frame) and the block partials of E = Re <psi|lambda>.
// Matrix elements as in k_s_energy: with d(p0) = sum_t s_t(p0) (cr_t + i ci_t) for the pair member p0 whose highest bit
// of x' is clear, lambda[p0 ^ x'] += d(p0) psi[p0] and lambda[p0] += conj(d(p0)) psi[p0 ^ x']; the sign sum is taken at
// p0 for both members.  The diagonal group multiplies by its real sign sum.
__global__ void __launch_bounds__(kThreads) k_sg_lambda(BatchArgs A, const double2* states, int n_terms,
                                                        const uint32_t* gxp, const uint32_t* tzp, const double* tsg,
                                                        double2* lambda, double* partial) {
  __shared__ double red[8];
  const int b = blockIdx.y;
  const size_t dim = (size_t)1 << A.n;
  const double2* psi = states + (size_t)b * dim;
  double2* lam = lambda + (size_t)b * dim;
  const uint32_t* gx = gxp + (size_t)b * A.ham.n_groups;
  const uint32_t* tz = tzp + (size_t)b * n_terms;
  const double* ts = tsg + (size_t)b * n_terms;
  const uint32_t base = blockIdx.x * (kThreads * kLambdaApt) + threadIdx.x;
  uint32_t p[kLambdaApt];
  bool in[kLambdaApt];
  double2 own[kLambdaApt], acc[kLambdaApt];
#pragma unroll
  for (int k = 0; k < kLambdaApt; ++k) {
    p[k] = base + (uint32_t)k * kThreads;
    in[k] = p[k] < dim;
    own[k] = in[k] ? psi[p[k]] : make_double2(0.0, 0.0);
    acc[k] = make_double2(0.0, 0.0);
  }
  for (int g = 0; g < A.ham.n_groups; ++g) {
    const uint32_t x = gx[g];
    const int t0 = A.ham.term_off[g], t1 = A.ham.term_off[g + 1];
    if (x == 0) {
      double d[kLambdaApt];
#pragma unroll
      for (int k = 0; k < kLambdaApt; ++k) d[k] = 0.0;
      for (int t = t0; t < t1; ++t) {
        const double c = ts[t] * A.ham.term_cr[t];
        const uint32_t z = tz[t];
#pragma unroll
        for (int k = 0; k < kLambdaApt; ++k) d[k] += parity32(p[k] & z) ? -c : c;
      }
#pragma unroll
      for (int k = 0; k < kLambdaApt; ++k) {
        acc[k].x += d[k] * own[k].x;
        acc[k].y += d[k] * own[k].y;
      }
    } else {
      const int hb = 31 - __clz((int)x);
      uint32_t p0[kLambdaApt];
      double2 a[kLambdaApt];
      double dr[kLambdaApt], di[kLambdaApt];
#pragma unroll
      for (int k = 0; k < kLambdaApt; ++k) {
        p0[k] = ((p[k] >> hb) & 1u) ? p[k] ^ x : p[k];
        a[k] = in[k] ? psi[p[k] ^ x] : make_double2(0.0, 0.0);
        dr[k] = di[k] = 0.0;
      }
      for (int t = t0; t < t1; ++t) {
        const double s = ts[t], cr = A.ham.term_cr[t], ci = A.ham.term_ci[t];
        const uint32_t z = tz[t];
#pragma unroll
        for (int k = 0; k < kLambdaApt; ++k) {
          const double sg = parity32(p0[k] & z) ? -s : s;
          dr[k] += sg * cr;
          di[k] += sg * ci;
        }
      }
#pragma unroll
      for (int k = 0; k < kLambdaApt; ++k) {
        const double im = ((p[k] >> hb) & 1u) ? di[k] : -di[k];      // d for the p0 ^ x' member, conj(d) for p0
        acc[k].x += dr[k] * a[k].x - im * a[k].y;
        acc[k].y += dr[k] * a[k].y + im * a[k].x;
      }
    }
  }
  double e = 0.0;
#pragma unroll
  for (int k = 0; k < kLambdaApt; ++k)
    if (in[k]) {
      lam[p[k]] = acc[k];
      e += own[k].x * acc[k].x + own[k].y * acc[k].y;
    }
  const double tot = block_sum(e, red);
  if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = tot;
}

// Backward sweep over the ops [o, o + K) of every stream: the slot-and-coset construction of k_s_opk (same reduce /
// push / flip basis), the thread's 2^K amplitudes of psi and of lambda in registers.  PZ: the streams hold OP_PZ records
// (a diagonal: no partner mask, so it sits in a filler slot as any op that is no pair op).
template <int K, bool PZ>
__device__ __forceinline__ void sg_back(const BatchArgs& A, double2* states, double2* lambda, const Op* ops,
                                        const int32_t* meta, const double2* cs, double* gpart, const int o) {
  constexpr int E = 1 << K;
  __shared__ double redsm[8];
  const int b = blockIdx.y;
  const int nops = meta[(size_t)b * 8];
  if (o >= nops) return;                                    // (block-uniform: the streams of a batch differ in length)
  const int cnt = nops - o < K ? nops - o : K;
  const size_t dim = (size_t)1 << A.n;
  double2* psi = states + (size_t)b * dim;
  double2* lam = lambda + (size_t)b * dim;
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  const bool live = t < (dim >> K);                         // (no early return: the block sums below hold barriers)
  Op op[K];
  uint32_t g[K], red[K];       // slot masks; the same span in reduced echelon form
  int hbit[K], flip[K];
  uint32_t pivots = 0;
  int nred = 0;
  auto reduce = [&](uint32_t x) {   // x modulo the span collected so far
#pragma unroll
    for (int i = 0; i < K; ++i) if (i < nred && ((x >> hbit[i]) & 1u)) x ^= red[i];
    return x;
  };
  auto push = [&](uint32_t x) {     // x != 0 reduced: new basis vector, keep the others reduced
    const int h = 31 - __clz((int)x);
#pragma unroll
    for (int i = 0; i < K; ++i) if (i < nred && ((red[i] >> h) & 1u)) red[i] ^= x;
#pragma unroll
    for (int i = 0; i < K; ++i) if (i == nred) { red[i] = x; hbit[i] = h; }
    pivots |= 1u << h;
    ++nred;
  };
  // pass 1: independent partner masks take their own slot
  bool own[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    own[j] = false;
    g[j] = 0;
    flip[j] = 0;
    red[j] = 0;
    hbit[j] = 0;
    op[j] = Op{0u, 0u, -1, OP_NOP};
    if (j < cnt) {
      op[j] = ops[(size_t)b * A.max_ops + o + j];
      const int k = op[j].kind & 0xff;
      if (op_is_pair(k)) {
        const uint32_t r = reduce(op[j].xm);
        if (r) { push(r); g[j] = op[j].xm; own[j] = true; flip[j] = 1 << j; }
      }
    }
  }
  // pass 2: fillers for the other slots
  {
    int q = 0;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (!own[j]) {
        uint32_t r = 0;
        while ((r = reduce(1u << q)) == 0) ++q;
        push(r);
        g[j] = 1u << q;
        ++q;
      }
  }
  // pass 3: flip codes of the dependent partner masks (brute force over the 2^K - 1 combinations)
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j < cnt && !own[j]) {
      const int k = op[j].kind & 0xff;
      if (op_is_pair(k))
#pragma unroll
        for (int f = 1; f < E; ++f) {
          uint32_t x = 0;
#pragma unroll
          for (int i = 0; i < K; ++i) if ((f >> i) & 1) x ^= g[i];
          if (x == op[j].xm) flip[j] = f;
        }
    }
  // coset representative: zeros inserted at the pivot bits, lowest first
  uint32_t p0 = live ? t : 0u;
  for (int q = 0; q < A.n; ++q) if ((pivots >> q) & 1u) p0 = insert0(p0, q);
  uint32_t idx[E];
  double2 v[E], l[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    uint32_t x = p0;
#pragma unroll
    for (int i = 0; i < K; ++i) if ((e >> i) & 1) x ^= g[i];
    idx[e] = x;
    v[e] = psi[x];
    l[e] = lam[x];
  }
  const double2* csb = cs + (size_t)b * A.max_params;
  const int P = A.par_count[b];
  double gp[K];
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {
    gp[j] = 0.0;
    const int kind = op[j].kind & 0xff;
    const bool rot = j < cnt && (op_is_pair(kind) || kind == OP_RZ) && op[j].pidx >= 0 && op[j].pidx < P;
    if (rot) {
      const double2 c = csb[op[j].pidx];
      double2 w[E];
#pragma unroll
      for (int e = 0; e < E; ++e) w[e] = v[e];
      s_apply_k_cs<K>(w, idx, op[j], make_double2(0.0, 1.0), flip[j]);      // K psi
      double acc = 0.0;
#pragma unroll
      for (int e = 0; e < E; ++e) acc += l[e].x * w[e].x + l[e].y * w[e].y;
      gp[j] = live ? acc : 0.0;
      const double2 ci = make_double2(c.x, -c.y);                           // U^-1
      s_apply_k_cs<K>(v, idx, op[j], ci, flip[j]);
      s_apply_k_cs<K>(l, idx, op[j], ci, flip[j]);
    } else if (PZ && j < cnt && kind == OP_PZ) {
      s_apply_k_cs<K, true>(v, idx, op[j], make_double2(1.0, 0.0), 0);
      s_apply_k_cs<K, true>(l, idx, op[j], make_double2(1.0, 0.0), 0);
    }
  }
  if (live) {
#pragma unroll
    for (int e = 0; e < E; ++e) { psi[idx[e]] = v[e]; lam[idx[e]] = l[e]; }
  }
  double* gout = gpart + ((size_t)b * A.max_ops + o) * gridDim.x + blockIdx.x;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j < cnt) {                                          // (block-uniform)
      const double tot = block_sum(gp[j], redsm);
      if (threadIdx.x == 0) gout[(size_t)j * gridDim.x] = tot;
    }
  }
}
template <int K>
__global__ void __launch_bounds__(kThreads) k_sg_back(BatchArgs A, double2* states, double2* lambda, const Op* ops,
                                                      const int32_t* meta, const double2* cs, double* gpart, int o) {
  sg_back<K, false>(A, states, lambda, ops, meta, cs, gpart, o);
}
template <int K>
__global__ void __launch_bounds__(kThreads) k_sg_back_pz(BatchArgs A, double2* states, double2* lambda, const Op* ops,
                                                         const int32_t* meta, const double2* cs, double* gpart, int o) {
  sg_back<K, true>(A, states, lambda, ops, meta, cs, gpart, o);
}

// grad[par_begin[b] + j]: one workgroup per (parameter, stream).  Thread i adds the partials i, i + 256, ... of every op
// with parameter j, op after op, and the block sum closes it - one fixed order whatever the launch.
__global__ void __launch_bounds__(kThreads) k_sg_reduce(BatchArgs A, const Op* ops, const int32_t* meta,
                                                        const double* gpart, int nblk, double* grad) {
  __shared__ double red[8];
  const int b = blockIdx.y, j = blockIdx.x;
  if (j >= A.par_count[b]) return;
  const int nops = meta[(size_t)b * 8];
  const Op* op = ops + (size_t)b * A.max_ops;
  double acc = 0.0;
  for (int o = 0; o < nops; ++o) {
    const int kind = op[o].kind & 0xff;
    if (op[o].pidx != j || !(op_is_pair(kind) || kind == OP_RZ)) continue;
    const double* src = gpart + ((size_t)b * A.max_ops + o) * nblk;
    for (int i = threadIdx.x; i < nblk; i += kThreads) acc += src[i];
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) grad[A.par_begin[b] + j] = tot;
}

// E (A.fout) and dE/dtheta (grad, the layout of the batch's theta) of every resident stream.
// keys: NULL, or the draw keys of the streams of a noisy chunk (stream_evaluate); the backward sweeps are then the
// instance that knows the OP_PZ record.
inline int stream_energy_grad(StreamWork& sw, const BatchArgs& A, hipStream_t st, uint64_t eval_id, double* grad,
                              std::string& err, uint64_t generation, const uint64_t* keys = nullptr) {
  constexpr int K = kGradOpsPerSweep;
  VQE_TRY(stream_evaluate(sw, A, st, eval_id, StreamWant::Circuit, err, generation, keys));
  const int n_terms = A.ham.n_terms;
  const size_t dim = (size_t)1 << A.n;
  const int B = A.batch;
  const int lblk = (int)((dim + (size_t)kThreads * kLambdaApt - 1) / ((size_t)kThreads * kLambdaApt));
  const int gblk = (int)(((dim >> K) + kThreads - 1) / kThreads);
  HIP_TRY(err, sw.lam.reserve((size_t)B * dim));
  HIP_TRY(err, sw.gpart.reserve((size_t)B * A.max_ops * gblk));
  HIP_TRY(err, sw.partial.reserve((size_t)B * lblk));
  const int nt = n_terms > 0 ? n_terms : 1, ng = A.ham.n_groups > 0 ? A.ham.n_groups : 1;
  hipLaunchKernelGGL(k_s_terms, dim3((std::max(nt, ng) + 63) / 64, B), dim3(64), 0, st, A, sw.masks.p, sw.meta.p, n_terms,
                     sw.gxp.p, sw.tzp.p, sw.tsg.p);
  hipLaunchKernelGGL(k_sg_lambda, dim3(lblk, B), dim3(kThreads), 0, st, A, (const double2*)sw.states.p, n_terms,
                     (const uint32_t*)sw.gxp.p, (const uint32_t*)sw.tzp.p, (const double*)sw.tsg.p, sw.lam.p, sw.partial.p);
  hipLaunchKernelGGL(k_s_reduce, dim3(B), dim3(kThreads), 0, st, sw.partial.p, lblk, A.fout, A.noise, eval_id, 0);
  const auto back = keys ? k_sg_back_pz<K> : k_sg_back<K>;
  for (int o = ((A.max_ops - 1) / K) * K; o >= 0; o -= K)      // the op groups of the forward sweeps, last first
    hipLaunchKernelGGL(back, dim3(gblk, B), dim3(kThreads), 0, st, A, sw.states.p, sw.lam.p, (const Op*)sw.ops.p,
                       (const int32_t*)sw.meta.p, (const double2*)sw.cs.p, sw.gpart.p, o);
  hipLaunchKernelGGL(k_sg_reduce, dim3(A.max_params, B), dim3(kThreads), 0, st, A, (const Op*)sw.ops.p,
                     (const int32_t*)sw.meta.p, (const double*)sw.gpart.p, gblk, grad);
  HIP_TRY(err, hipGetLastError());
  return 0;
}

// ---- the mean over frozen Pauli-noise realisations (vqe_set_stream_noise_grad) ------------------------
// Buffers of the expanded batch of a chunk (sized by the resident count) and the per-pair results of a run (B * T rows).
struct StreamNoiseWork {
  DevBufExact<int64_t> gbeg, pbeg;      // [resident] gate range of the pair's circuit; its theta slot i * max_params
  DevBufExact<int32_t> gcnt, pcnt;      // [resident]
  DevBufExact<uint64_t> keys;           // [resident][2] (b, eval_base + t)
  DevBufExact<double> theta;            // [resident][max_params]
  DevBufExact<double> pair_e, pair_g;   // [B * T], [B * T][max_params]
};

// The index arrays of the pairs v0 .. v0 + cnt - 1 (v = b * T + t): one thread per pair.
__global__ void k_sn_expand(BatchArgs A, int T, int64_t v0, int cnt, uint64_t eval_base, int64_t* gbeg, int32_t* gcnt,
                            int64_t* pbeg, int32_t* pcnt, uint64_t* keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const int64_t v = v0 + i;
  const int b = (int)(v / T), t = (int)(v % T);
  gbeg[i] = A.gate_begin[b];
  gcnt[i] = A.gate_count[b];
  pbeg[i] = (int64_t)i * A.max_params;
  pcnt[i] = A.par_count[b];
  keys[2 * (size_t)i] = (uint64_t)b;
  keys[2 * (size_t)i + 1] = eval_base + (uint64_t)t;
}
// theta of circuit b to the slot of each of its pairs in the chunk (at every evaluation: an optimiser moves theta)
__global__ void k_sn_theta(BatchArgs A, int T, int64_t v0, double* theta_x) {
  const int i = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = (int)((v0 + i) / T);
  if (j >= A.par_count[b]) return;
  theta_x[(size_t)i * A.max_params + j] = A.theta[A.par_begin[b] + j];
}
// E_T[b] (thread j == max_params) and grad[par_begin[b] + j]: the T per-pair values added in ascending t, divided once.
__global__ void k_sg_mean(BatchArgs A, int T, const double* pair_e, const double* pair_g, double* fout, double* grad) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t v = (size_t)b * T;
  if (j == A.max_params) {
    double acc = 0.0;
    for (int t = 0; t < T; ++t) acc += pair_e[v + t];
    fout[b] = acc / (double)T;
  } else if (j < A.par_count[b]) {
    double acc = 0.0;
    for (int t = 0; t < T; ++t) acc += pair_g[(v + t) * A.max_params + j];
    grad[A.par_begin[b] + j] = acc / (double)T;
  }
}

// E_T (A.fout) and its gradient (grad, the layout of the batch's theta) of the batch A describes, at A.theta: the pairs of
// every chunk as streams of one stream_energy_grad, then the mean.  cap: resident pairs asked for; *used / *chunks: out.
inline int stream_noise_energy_grad(StreamWork& sw, StreamNoiseWork& nw, const BatchArgs& A, hipStream_t st, uint64_t eval_base,
                                    int T, int64_t cap, double* grad, std::string& err, uint64_t generation, int* used,
                                    int* chunks) {
  const NoiseGradChunks P = noise_grad_chunks(A.batch, T, cap);
  const int R = P.resident, mp = A.max_params;
  *used = R;
  *chunks = P.chunks;
  HIP_TRY(err, nw.gbeg.reserve(R));
  HIP_TRY(err, nw.pbeg.reserve(R));
  HIP_TRY(err, nw.gcnt.reserve(R));
  HIP_TRY(err, nw.pcnt.reserve(R));
  HIP_TRY(err, nw.keys.reserve((size_t)2 * R));
  HIP_TRY(err, nw.theta.reserve((size_t)R * std::max(mp, 1)));
  HIP_TRY(err, nw.pair_e.reserve((size_t)std::max<int64_t>(P.pairs, 1)));
  HIP_TRY(err, nw.pair_g.reserve((size_t)std::max<int64_t>(P.pairs, 1) * std::max(mp, 1)));
  for (int c = 0; c < P.chunks; ++c) {
    int64_t lo, hi;
    noise_grad_chunk_range(P, c, &lo, &hi);
    const int cnt = (int)(hi - lo);
    hipLaunchKernelGGL(k_sn_expand, dim3((cnt + 63) / 64), dim3(64), 0, st, A, T, lo, cnt, eval_base, nw.gbeg.p, nw.gcnt.p,
                       nw.pbeg.p, nw.pcnt.p, nw.keys.p);
    hipLaunchKernelGGL(k_sn_theta, dim3((std::max(mp, 1) + 63) / 64, cnt), dim3(64), 0, st, A, T, lo, nw.theta.p);
    BatchArgs C = A;
    C.batch = cnt;
    C.gate_begin = nw.gbeg.p; C.gate_count = nw.gcnt.p;
    C.par_begin = nw.pbeg.p; C.par_count = nw.pcnt.p;
    C.theta = nw.theta.p;
    C.fout = nw.pair_e.p + lo;
    VQE_TRY(stream_energy_grad(sw, C, st, eval_base, nw.pair_g.p + (size_t)lo * mp, err, generation, (const uint64_t*)nw.keys.p));
  }
  hipLaunchKernelGGL(k_sg_mean, dim3((mp + 1 + 63) / 64, A.batch), dim3(64), 0, st, A, T, (const double*)nw.pair_e.p,
                     (const double*)nw.pair_g.p, A.fout, grad);
  HIP_TRY(err, hipGetLastError());
  return 0;
}

}  // namespace vqe
