// vqe_stream_qjump.h - quantum-jump trajectories of a Kraus channel on the streaming path (n >= 14), opt-in per handle
// (vqe_set_stream_kraus_traj).  The trajectory is the one vqe_qjump.h defines: the same draw, selection rule and counters.
//
// A (circuit, trajectory) work item w = b T + t is a virtual stream with its own 2^n complex128 state in HBM; a chunk of
// `cnt` of them is resident at a time.  All T trajectories of a circuit share its compiled records and frame
// (k_sq_compile: qj_compile, one thread per circuit).  The resident streams run in lock-step rounds (stream_qjump_host.h):
//   round r:  the r-th run of rotation records, kSqOpsPerSweep per read-modify-write sweep    (k_sq_rot)
//             rho_red of the r-th jump: one read-only sweep, one partial row per workgroup       (k_sq_partial)
//             the selection, one wavefront per stream: the rows summed in index order, p_k, the draw, k,
//             K_k / sqrt(p_k) into the stream's slot                                              (k_sq_select)
//             psi <- K_k psi / sqrt(p_k) as a general pair or quad op in the frame                (k_sq_apply)
// A stream with fewer jumps than the round idles (its workgroups return).  The host queues launches only: their number
// depends on the circuits (rounds, longest run), not on the batch, T or the chunk.  The energies of the chunk are the
// streaming path's own Pauli-term reduction on the virtual batch (stream_evaluate, vqe_stream.h) with the frame below.
//
// Bits: a workgroup of k_sq_partial owns kSqGroups consecutive coset representatives of its stream, whatever the grid
// around it; its 4 or 16 sums are reduced in a fixed order (qj_block_sum), the rows of a stream are added in index order
// by one lane per real, and every lane of the selecting wavefront computes the same k from the same numbers.  No atomics.
// Nothing depends on the chunk, the batch around a circuit or the device's occupancy.
#pragma once
#include "stream_qjump_host.h"

#if defined(__HIPCC__)
namespace vqe {

struct SqDev {
  int n, T;
  int cnt;                  // resident virtual streams of this chunk
  long long w0;             // ... which are the work items w0 .. w0 + cnt - 1
  double2* states;          // [cnt][2^n]
  const double2* init;      // [2^n]
  const QjOp* ops;          // [batch][max_ops]
  const int32_t* meta;      // [batch][8]: records, c of the frame, 0 (no phase), jumps
  const int32_t* jpos;      // [batch][max_ops] positions of the jump records
  const double2* cs;        // [batch][max_params] (cos, sin) of theta / 2
  int max_ops, max_params;
  double* part;             // [cnt][blocks][16] partial rows of rho_red
  double* kmat;             // [cnt][32] K_k / sqrt(p_k) of the jump in flight, (re, im) row major
  int32_t* jumps;           // [batch * T] selections k != 0, zeroed by the caller before the first chunk
  int n1, n2;               // the channel tables of the handle (qj_prepare)
  const double *K1, *W1, *K2, *W2;
  uint64_t seed, eval_id;
};

constexpr int kSqGroups = 2048;      // pairs or quads of a workgroup of the sweeps: 8 per thread
inline int sq_blocks(int n) { return (int)((((size_t)1 << n) / 2) / kSqGroups); }      // workgroups per stream (n >= 13)
inline size_t sq_state_sweeps(const SqSize& s) { return (size_t)1 + (size_t)(s.rounds + 1) * s.sweeps + (size_t)2 * s.rounds; }

// Defined in vqe_qjump.hip, beside the LDS path's kernels whose helpers they share.  All queue on `stream`.
// sq_compile: records, frame (masks: [batch][64] xm, zm; meta), jump positions and (cos, sin) of every circuit of A.
hipError_t sq_compile(const BatchArgs& A, bool slot1, bool slot2, QjOp* ops, uint32_t* masks, int32_t* meta, int32_t* jpos,
                      double2* cs, hipStream_t stream);
// sq_trajectories: the chunk D from the initial state through all rounds; *grid: workgroups of the last sweep.
hipError_t sq_trajectories(const SqDev& D, const SqSize& size, hipStream_t stream, int* grid);
// sq_frames: the frame of every stream of the chunk in the layout of k_s_terms / k_s_state_out ([cnt][64], [cnt][8]).
hipError_t sq_frames(const SqDev& D, const uint32_t* masks, uint32_t* vmasks, int32_t* vmeta, hipStream_t stream);
// sq_mean: k_qj_mean over the per-trajectory energies.
hipError_t sq_mean(int batch, int T, const double* etraj, const int32_t* jumps, const int32_t* active, NoiseCfg noise,
                   uint64_t eval_id, double* fout, int32_t* nfev, long long* jsum, hipStream_t stream);

}  // namespace vqe
#endif  // __HIPCC__

#if defined(__HIPCC__) && defined(VQE_QJUMP_KERNELS)      // (vqe_qjump.hip)
namespace vqe {

__global__ void k_sq_compile(BatchArgs A, int slot1, int slot2, QjOp* ops, uint32_t* masks, int32_t* meta, int32_t* jpos) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= A.batch) return;
  uint32_t* xm = masks + (size_t)b * 64;
  QjOp* out = ops + (size_t)b * A.max_ops;
  uint32_t c = 0;
  int nops = qj_compile(A.gates + A.gate_begin[b], A.gate_count[b], A.n, slot1 != 0, slot2 != 0, out, A.max_ops, xm, xm + 32, &c);
  if (nops > A.max_ops) nops = 0;      // (the host sizes max_ops by the batch: a list that does not fit is not run)
  int32_t* m = meta + (size_t)b * 8;
  m[0] = nops;
  m[1] = (int32_t)c;
  m[2] = 0;
  m[3] = sq_jump_positions(out, nops, jpos + (size_t)b * A.max_ops, A.max_ops);
}

__global__ void k_sq_sincos(BatchArgs A, double2* cs) {
  const int b = blockIdx.y;
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= A.par_count[b]) return;
  double s, c;
  sincos(0.5 * A.theta[A.par_begin[b] + j], &s, &c);
  cs[(size_t)b * A.max_params + j] = make_double2(c, s);
}

__global__ void __launch_bounds__(kThreads) k_sq_init(SqDev D) {
  const size_t dim = (size_t)1 << D.n;
  const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (p < dim) D.states[(size_t)blockIdx.y * dim + p] = D.init[p];
}

__global__ void k_sq_frames(SqDev D, const uint32_t* masks, uint32_t* vmasks, int32_t* vmeta) {
  const int s = blockIdx.x, b = (int)((D.w0 + s) / D.T);
  vmasks[(size_t)s * 64 + threadIdx.x] = masks[(size_t)b * 64 + threadIdx.x];
  if (threadIdx.x < 8) vmeta[(size_t)s * 8 + threadIdx.x] = D.meta[(size_t)b * 8 + threadIdx.x];
}

// sweep `sweep` of the rotation run of round r: one record, one pair (RZ: two neighbours) per thread and step
__global__ void __launch_bounds__(kThreads) k_sq_rot(SqDev D, int r, int sweep) {
  const int s = blockIdx.y, b = (int)((D.w0 + s) / D.T);
  const int32_t* m = D.meta + (size_t)b * 8;
  const int nops = m[0], njump = m[3];
  if (r > njump) return;
  const QjOp* ops = D.ops + (size_t)b * D.max_ops;
  int lo, hi;
  sq_round(ops, nops, D.jpos + (size_t)b * D.max_ops, njump, r, &lo, &hi);
  const int o = lo + sweep * kSqOpsPerSweep;
  if (o >= hi) return;
  const QjOp op = ops[o];
  const int kind = op.kind & 0xff, inv = (op.kind >> 8) & 1;
  const double2 cs = D.cs[(size_t)b * D.max_params + op.arg];
  double2* psi = D.states + ((size_t)s << D.n);
  const uint32_t q0 = blockIdx.x * (uint32_t)kSqGroups + threadIdx.x;
  if (op_is_pair(kind)) {
    const int hb = 31 - __clz((int)op.xm);
#pragma unroll
    for (int k = 0; k < kSqGroups / kThreads; ++k) {
      const uint32_t p0 = insert0(q0 + (uint32_t)k * kThreads, hb), p1 = p0 ^ op.xm;
      const double2 a0 = psi[p0], a1 = psi[p1];
      if (kind == OP_RX) {
        psi[p0] = make_double2(cs.x * a0.x - cs.y * a1.y, cs.x * a0.y + cs.y * a1.x);
        psi[p1] = make_double2(cs.x * a1.x - cs.y * a0.y, cs.x * a1.y + cs.y * a0.x);
      } else if (kind == OP_RY) {
        const double s0 = (parity32(p0 & op.zm) ^ inv) ? -cs.y : cs.y;
        psi[p0] = make_double2(cs.x * a0.x + s0 * a1.x, cs.x * a0.y + s0 * a1.y);
        psi[p1] = make_double2(cs.x * a1.x - s0 * a0.x, cs.x * a1.y - s0 * a0.y);
      } else {   // OP_RYY
        const double s0 = (parity32(p0 & op.zm) ^ inv) ? cs.y : -cs.y;
        psi[p0] = make_double2(cs.x * a0.x - s0 * a1.y, cs.x * a0.y + s0 * a1.x);
        psi[p1] = make_double2(cs.x * a1.x - s0 * a0.y, cs.x * a1.y + s0 * a0.x);
      }
    }
  } else if (kind == OP_RZ) {
#pragma unroll
    for (int k = 0; k < kSqGroups / kThreads; ++k) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t p = 2u * (q0 + (uint32_t)k * kThreads) + (uint32_t)j;
        const double sg = (parity32(p & op.zm) ^ inv) ? -cs.y : cs.y;
        const double2 a = psi[p];
        psi[p] = make_double2(cs.x * a.x - sg * a.y, cs.x * a.y + sg * a.x);
      }
    }
  }
}

// rho_red of the jump of round r: the reals of vqe_qjump.h, one row of 16 per workgroup (one-qubit jump: the first 4)
__global__ void __launch_bounds__(kThreads) k_sq_partial(SqDev D, int r) {
  __shared__ double red[(kThreads / 64) * 16];
  const int s = blockIdx.y, b = (int)((D.w0 + s) / D.T);
  const int32_t* m = D.meta + (size_t)b * 8;
  if (r >= m[3]) return;
  const QjOp* ops = D.ops + (size_t)b * D.max_ops;
  const int o = D.jpos[(size_t)b * D.max_ops + r];
  const QjOp op = ops[o];
  const int inv = (op.kind >> 8) & 1;
  const double2* psi = D.states + ((size_t)s << D.n);
  double* row = D.part + ((size_t)s * gridDim.x + blockIdx.x) * 16;
  const uint32_t q0 = blockIdx.x * (uint32_t)kSqGroups + threadIdx.x;
  if ((op.kind & 0xff) == QJ_JUMP1) {
    const int hb = 31 - __clz((int)op.xm);
    double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kSqGroups / kThreads; ++k) {
      const uint32_t p0 = insert0(q0 + (uint32_t)k * kThreads, hb);
      double2 a0 = psi[p0], a1 = psi[p0 ^ op.xm];
      qj_swap((parity32(p0 & op.zm) ^ inv) != 0, a0, a1);
      v[0] += a0.x * a0.x + a0.y * a0.y;
      v[1] += a1.x * a1.x + a1.y * a1.y;
      v[2] += a1.x * a0.x + a1.y * a0.y;
      v[3] += a1.y * a0.x - a1.x * a0.y;
    }
    qj_block_sum<kThreads / 64, 4>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) row[j] = v[j];
    }
    return;
  }
  // QJ_JUMP2: a quarter of the state's indices are representatives - the upper half of the grid writes rows of zeros
  const QjOp ob = ops[o + 1];
  const int invb = (op.kind >> 9) & 1;
  double v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = 0.0;
  if (blockIdx.x < gridDim.x / 2) {
    int lo, hi;
    qj_quad_bits(op.xm, ob.xm, &lo, &hi);
#pragma unroll
    for (int k = 0; k < kSqGroups / kThreads; ++k) {
      const uint32_t p = insert0(insert0(q0 + (uint32_t)k * kThreads, lo), hi);
      double2 a[4] = {psi[p], psi[p ^ op.xm], psi[p ^ ob.xm], psi[p ^ op.xm ^ ob.xm]};
      const bool s0 = (parity32(p & op.zm) ^ inv) != 0, s1 = (parity32(p & ob.zm) ^ invb) != 0;
      qj_swap(s0, a[0], a[1]); qj_swap(s0, a[2], a[3]);
      qj_swap(s1, a[0], a[2]); qj_swap(s1, a[1], a[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += a[i].x * a[i].x + a[i].y * a[i].y;
      int tt = 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = i + 1; j < 4; ++j) {
          v[tt++] += a[j].x * a[i].x + a[j].y * a[i].y;
          v[tt++] += a[j].y * a[i].x - a[j].x * a[i].y;
        }
      }
    }
    qj_block_sum<kThreads / 64, 16>(v, red);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) row[j] = v[j];
  }
}

// one wavefront per stream: the rows in index order, the selection rule, the jump count, K_k / sqrt(p_k)
__global__ void __launch_bounds__(64) k_sq_select(SqDev D, int r, int blocks) {
  __shared__ double rs[16];
  const int s = blockIdx.x;
  const long long w = D.w0 + s;
  const int b = (int)(w / D.T), t = (int)(w % D.T);
  const int32_t* m = D.meta + (size_t)b * 8;
  if (r >= m[3]) return;
  const QjOp op = D.ops[(size_t)b * D.max_ops + D.jpos[(size_t)b * D.max_ops + r]];
  const bool two = (op.kind & 0xff) == QJ_JUMP2;
  const int nr = two ? 16 : 4;
  const int lane = (int)threadIdx.x;
  if (lane < nr) {
    const double* col = D.part + (size_t)s * blocks * 16 + lane;
    double acc = 0.0;
    for (int i = 0; i < blocks; ++i) acc += col[(size_t)i * 16];
    rs[lane] = acc;
  }
  __syncthreads();
  const double u = noise_uniform_k(noise_key(D.seed, (uint64_t)b, D.eval_id), ((uint64_t)(t + 1) << 44) | (uint64_t)(uint32_t)op.arg);
  double scale;
  int ks;
  if (two) {
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = rs[j];
    ks = qj_select<16>(v, D.W2, D.n2, u, &scale);
    if (lane < 32) D.kmat[(size_t)s * 32 + lane] = D.K2[(size_t)ks * 32 + lane] * scale;
  } else {
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = rs[j];
    ks = qj_select<4>(v, D.W1, D.n1, u, &scale);
    if (lane < 8) D.kmat[(size_t)s * 32 + lane] = D.K1[(size_t)ks * 8 + lane] * scale;
  }
  if (lane == 0 && ks != 0) D.jumps[w] += 1;      // (this wavefront is the only writer of the slot)
}

// psi <- (K_k / sqrt(p_k)) psi on the jump's qubits, in the frame
__global__ void __launch_bounds__(kThreads) k_sq_apply(SqDev D, int r) {
  const int s = blockIdx.y, b = (int)((D.w0 + s) / D.T);
  const int32_t* m = D.meta + (size_t)b * 8;
  if (r >= m[3]) return;
  const QjOp* ops = D.ops + (size_t)b * D.max_ops;
  const int o = D.jpos[(size_t)b * D.max_ops + r];
  const QjOp op = ops[o];
  const int inv = (op.kind >> 8) & 1;
  double2* psi = D.states + ((size_t)s << D.n);
  const double* __restrict__ kk = D.kmat + (size_t)s * 32;
  const uint32_t q0 = blockIdx.x * (uint32_t)kSqGroups + threadIdx.x;
  if ((op.kind & 0xff) == QJ_JUMP1) {
    const int hb = 31 - __clz((int)op.xm);
#pragma unroll
    for (int k = 0; k < kSqGroups / kThreads; ++k) {
      const uint32_t p0 = insert0(q0 + (uint32_t)k * kThreads, hb), p1 = p0 ^ op.xm;
      const bool sw = (parity32(p0 & op.zm) ^ inv) != 0;
      double2 a0 = psi[p0], a1 = psi[p1];
      qj_swap(sw, a0, a1);
      const double2 x0 = qj_cmul(kk[0], kk[1], a0), x1 = qj_cmul(kk[2], kk[3], a1);
      const double2 y0 = qj_cmul(kk[4], kk[5], a0), y1 = qj_cmul(kk[6], kk[7], a1);
      double2 n0 = make_double2(x0.x + x1.x, x0.y + x1.y), n1 = make_double2(y0.x + y1.x, y0.y + y1.y);
      qj_swap(sw, n0, n1);
      psi[p0] = n0;
      psi[p1] = n1;
    }
    return;
  }
  if (blockIdx.x >= gridDim.x / 2) return;
  const QjOp ob = ops[o + 1];
  const int invb = (op.kind >> 9) & 1;
  int lo, hi;
  qj_quad_bits(op.xm, ob.xm, &lo, &hi);
#pragma unroll
  for (int k = 0; k < kSqGroups / kThreads; ++k) {
    const uint32_t p = insert0(insert0(q0 + (uint32_t)k * kThreads, lo), hi);
    double2 a[4] = {psi[p], psi[p ^ op.xm], psi[p ^ ob.xm], psi[p ^ op.xm ^ ob.xm]};
    const bool s0 = (parity32(p & op.zm) ^ inv) != 0, s1 = (parity32(p & ob.zm) ^ invb) != 0;
    qj_swap(s0, a[0], a[1]); qj_swap(s0, a[2], a[3]);
    qj_swap(s1, a[0], a[2]); qj_swap(s1, a[1], a[3]);
    double2 nv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double2 acc = make_double2(0.0, 0.0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double2 t = qj_cmul(kk[(i * 4 + j) * 2], kk[(i * 4 + j) * 2 + 1], a[j]);
        acc.x += t.x; acc.y += t.y;
      }
      nv[i] = acc;
    }
    qj_swap(s1, nv[0], nv[2]); qj_swap(s1, nv[1], nv[3]);
    qj_swap(s0, nv[0], nv[1]); qj_swap(s0, nv[2], nv[3]);
    psi[p] = nv[0];
    psi[p ^ op.xm] = nv[1];
    psi[p ^ ob.xm] = nv[2];
    psi[p ^ op.xm ^ ob.xm] = nv[3];
  }
}

hipError_t sq_compile(const BatchArgs& A, bool slot1, bool slot2, QjOp* ops, uint32_t* masks, int32_t* meta, int32_t* jpos,
                      double2* cs, hipStream_t stream) {
  hipLaunchKernelGGL(k_sq_compile, dim3((unsigned)((A.batch + 63) / 64)), dim3(64), 0, stream, A, slot1 ? 1 : 0, slot2 ? 1 : 0, ops,
                     masks, meta, jpos);
  hipLaunchKernelGGL(k_sq_sincos, dim3((unsigned)((A.max_params + 63) / 64), (unsigned)A.batch), dim3(64), 0, stream, A, cs);
  return hipGetLastError();
}

hipError_t sq_trajectories(const SqDev& D, const SqSize& size, hipStream_t stream, int* grid) {
  const size_t dim = (size_t)1 << D.n;
  const unsigned blocks = (unsigned)sq_blocks(D.n), cnt = (unsigned)D.cnt;
  hipLaunchKernelGGL(k_sq_init, dim3((unsigned)(dim / kThreads), cnt), dim3(kThreads), 0, stream, D);
  *grid = (int)((dim / kThreads) * cnt);
  for (int r = 0; r <= size.rounds; ++r) {
    for (int s = 0; s < size.sweeps; ++s) hipLaunchKernelGGL(k_sq_rot, dim3(blocks, cnt), dim3(kThreads), 0, stream, D, r, s);
    if (r == size.rounds) break;
    hipLaunchKernelGGL(k_sq_partial, dim3(blocks, cnt), dim3(kThreads), 0, stream, D, r);
    hipLaunchKernelGGL(k_sq_select, dim3(cnt), dim3(64), 0, stream, D, r, (int)blocks);
    hipLaunchKernelGGL(k_sq_apply, dim3(blocks, cnt), dim3(kThreads), 0, stream, D, r);
  }
  if (size.rounds > 0 || size.sweeps > 0) *grid = (int)(blocks * cnt);
  return hipGetLastError();
}

hipError_t sq_frames(const SqDev& D, const uint32_t* masks, uint32_t* vmasks, int32_t* vmeta, hipStream_t stream) {
  hipLaunchKernelGGL(k_sq_frames, dim3((unsigned)D.cnt), dim3(64), 0, stream, D, masks, vmasks, vmeta);
  return hipGetLastError();
}

hipError_t sq_mean(int batch, int T, const double* etraj, const int32_t* jumps, const int32_t* active, NoiseCfg noise,
                   uint64_t eval_id, double* fout, int32_t* nfev, long long* jsum, hipStream_t stream) {
  hipLaunchKernelGGL(k_qj_mean, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, stream, batch, T, etraj, jumps, active, noise,
                     eval_id, fout, nfev, jsum);
  return hipGetLastError();
}

}  // namespace vqe
#endif  // VQE_QJUMP_KERNELS
