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
// Noise is refused before this path is entered (vqe_api.hip: grad_refusal), so ops other than rotations do not occur;
// an op of any other kind is skipped.
#pragma once
#include "vqe_stream.h"

namespace vqe {

constexpr int kGradOpsPerSweep = 3;   // K of k_sg_back: the largest that compiles for gfx950 without scratch
constexpr int kLambdaApt = 2;         // amplitudes a thread of k_sg_lambda owns

// s_apply_k with the angle given as (cos, sin) instead of read from the parameter table, and with the dependent-mask
// case spelled out per flip code (static register indices only: no scratch).  Ops that are no rotation are skipped.
template <int K>
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
// push / flip basis), the thread's 2^K amplitudes of psi and of lambda in registers.
template <int K>
__global__ void __launch_bounds__(kThreads) k_sg_back(BatchArgs A, double2* states, double2* lambda, const Op* ops,
                                                      const int32_t* meta, const double2* cs, double* gpart, int o) {
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
inline int stream_energy_grad(StreamWork& sw, const BatchArgs& A, hipStream_t st, uint64_t eval_id, double* grad,
                              std::string& err, uint64_t generation) {
  constexpr int K = kGradOpsPerSweep;
  VQE_TRY(stream_evaluate(sw, A, st, eval_id, StreamWant::Circuit, err, generation));
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
  for (int o = ((A.max_ops - 1) / K) * K; o >= 0; o -= K)      // the op groups of the forward sweeps, last first
    hipLaunchKernelGGL(k_sg_back<K>, dim3(gblk, B), dim3(kThreads), 0, st, A, sw.states.p, sw.lam.p, (const Op*)sw.ops.p,
                       (const int32_t*)sw.meta.p, (const double2*)sw.cs.p, sw.gpart.p, o);
  hipLaunchKernelGGL(k_sg_reduce, dim3(A.max_params, B), dim3(kThreads), 0, st, A, (const Op*)sw.ops.p,
                     (const int32_t*)sw.meta.p, (const double*)sw.gpart.p, gblk, grad);
  HIP_TRY(err, hipGetLastError());
  return 0;
}

}  // namespace vqe
