// vqe_qjump.h - quantum-jump trajectories of a Kraus channel on the LDS-resident state-vector path (1 <= n <= 13).
//
// vqe_set_kraus_traj(T >= 1) lets mode 0 run under a Kraus override (vqe_set_noise_kraus): an energy is the mean of T
// stochastic state-vector trajectories.  At a noise gate on qubits (q0[, q1]) with Kraus set {K_k}:
//   rho_red = the reduced density matrix of those qubits (2 x 2 or 4 x 4, index = bit(q0) + 2 bit(q1)),
//   p_k = tr(K_k^+ K_k rho_red)                                  (M_k = K_k^+ K_k is made once per override, on the host)
//   u   = noise_uniform_k(noise_key(seed, b, e), ((uint64_t)(t + 1) << 44) | g)
//         (stream b, evaluation e, trajectory t, g the position of the noise gate in the executed gate list)
//   k   = the smallest k with u < p_0 + ... + p_k (accumulated in k order in double); none (rounding): the last k with
//         p_k > 0
//   psi <- K_k psi / sqrt(p_k).
// The energy of an evaluation is the mean over t = 0 .. T-1 of <psi_t|H|psi_t>, summed in t order (k_qj_mean), plus
// shot_sigma * noise_gauss(seed, b, e) once per evaluation.
//
// One workgroup per (circuit, trajectory) in the Geo<N> geometry, a persistent grid over the B * T work items, psi
// LDS-resident for the whole trajectory.  The circuit is compiled once per circuit a workgroup meets into the GF(2)
// frame of compile_ops (vqe_device.h) by a walk of its own, qj_compile, which also builds for the host: the amplitude of
// logical index i lives at the frame index p with i = A p ^ c, row a of A = zm[a], column a of A^-1 = xm[a], so
//   bit of qubit a at frame index p = parity(p & zm[a]) ^ c_a,  flipping qubit a = p ^ xm[a],  zm[a] . xm[b] = delta_ab;
// a CNOT only updates the map.  A local operator on qubit a (a, b) therefore mixes {p, p ^ xm[a] (, p ^ xm[b],
// p ^ xm[a] ^ xm[b])}, and the local index of each member is read off the parities.  A jump takes two passes over the
// state: the 4 (one qubit: rho_00, rho_11, Re rho_10, Im rho_10) or 16 real numbers of rho_red in a fixed-order
// workgroup reduction, then - every thread computes the same k from the same reduced values - the application of
// K_k / sqrt(p_k) as a general 2 x 2 pair op or 4 x 4 quad op.  The energy is step 2 of the adjoint evaluation
// (vqe_grad_energy.h) on the GradHam tables.  Nothing in here depends on the batch around a work item: the same seed,
// counter, batch position and T give the same bits.
#pragma once
#include <stdint.h>
#include <complex>
#include <vector>
#include "vqe_geo.h"

namespace vqe {

// Records of the compiled trajectory, in the layout of Op (vqe_device.h).  Rotations as compile_ops leaves them (kind =
// OP_RX / OP_RY / OP_RZ / OP_RYY, whose numbers are those of the gate kinds; arg = parameter index; bit 8 = sign bit).
// QJ_JUMP1: xm / zm / bit 8 = c of the gate's qubit, arg = g.  QJ_JUMP2: the same for q0, bit 9 = c of q1, followed by a
// QJ_TAIL record with xm / zm of q1.
enum : int { QJ_JUMP1 = 8, QJ_JUMP2 = 9, QJ_TAIL = 10 };
struct QjOp { uint32_t xm, zm; int32_t arg; int32_t kind; };

// The walk.  slot1 / slot2: the one- / two-qubit noise slot holds a channel (an identity slot leaves no record).
// Writes at most cap records; returns the number the circuit needs.  xm, zm: [n] out, *c_out the offset of the frame.
VQE_HD inline int qj_compile(const GateRec* g, int G, int n, bool slot1, bool slot2, QjOp* ops, int cap, uint32_t* xm,
                             uint32_t* zm, uint32_t* c_out) {
  for (int q = 0; q < n; ++q) { xm[q] = 1u << q; zm[q] = 1u << q; }
  uint32_t c = 0;
  int nops = 0;
  for (int i = 0; i < G; ++i) {
    const GateRec r = g[i];
    switch (r.kind) {
      case G_CNOT:
        zm[r.q1] ^= zm[r.q0];
        xm[r.q0] ^= xm[r.q1];
        if ((c >> r.q0) & 1u) c ^= 1u << r.q1;
        break;
      case G_RX: case G_RY: case G_RZ:
        if (nops < cap) ops[nops] = QjOp{xm[r.q0], zm[r.q0], r.pidx, r.kind | (int)(((c >> r.q0) & 1u) << 8)};
        ++nops;
        break;
      case G_RXX: case G_RYY: case G_RZZ:
        if (nops < cap)
          ops[nops] = QjOp{xm[r.q0] ^ xm[r.q1], zm[r.q0] ^ zm[r.q1], r.pidx,
                           (r.kind == G_RXX ? G_RX : (r.kind == G_RYY ? G_RYY : G_RZ)) | (int)((((c >> r.q0) ^ (c >> r.q1)) & 1u) << 8)};
        ++nops;
        break;
      case G_DEPOL1:
        if (!slot1) break;
        if (nops < cap) ops[nops] = QjOp{xm[r.q0], zm[r.q0], i, QJ_JUMP1 | (int)(((c >> r.q0) & 1u) << 8)};
        ++nops;
        break;
      case G_DEPOL2:
        if (!slot2) break;
        if (nops + 1 < cap) {
          ops[nops] = QjOp{xm[r.q0], zm[r.q0], i, QJ_JUMP2 | (int)(((c >> r.q0) & 1u) << 8) | (int)(((c >> r.q1) & 1u) << 9)};
          ops[nops + 1] = QjOp{xm[r.q1], zm[r.q1], i, QJ_TAIL};
        }
        nops += 2;
        break;
      default: break;
    }
  }
  *c_out = c;
  return nops;
}

// The representatives of the cosets of span{xa, xb} (xa, xb independent): the indices whose bits *lo < *hi are both 0.
VQE_HD inline void qj_quad_bits(uint32_t xa, uint32_t xb, int* lo, int* hi) {
  int ha = 0, hb = 0;
  for (int q = 0; q < 32; ++q) if ((xa >> q) & 1u) ha = q;
  const uint32_t xr = ((xb >> ha) & 1u) ? xb ^ xa : xb;
  for (int q = 0; q < 32; ++q) if ((xr >> q) & 1u) hb = q;
  *lo = ha < hb ? ha : hb;
  *hi = ha < hb ? hb : ha;
}

// Host tables of a Kraus set of `count` d x d operators (d = 2, 4; row major, as vqe_set_noise_kraus takes them):
// K as (re, im) pairs and, per operator, the weights w of p_k = sum_j w[j] r[j] over the reduced reals r of rho_red:
//   r[i] = rho_ii (i < d), then for the pairs i < j in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3): Re rho_ji, Im rho_ji;
//   w[i] = M_ii, then 2 Re M_ij, -2 Im M_ij, with M = K^+ K  (tr(M rho) = sum_i M_ii rho_ii + 2 sum_{i<j} Re(M_ij rho_ji)).
inline void qj_build_tables(const std::complex<double>* K, int count, int d, std::vector<double>& k_out, std::vector<double>& w_out) {
  const int nr = d * d;
  k_out.assign((size_t)count * nr * 2, 0.0);
  w_out.assign((size_t)count * nr, 0.0);
  for (int k = 0; k < count; ++k) {
    const std::complex<double>* Kk = K + (size_t)k * nr;
    for (int e = 0; e < nr; ++e) { k_out[((size_t)k * nr + e) * 2] = Kk[e].real(); k_out[((size_t)k * nr + e) * 2 + 1] = Kk[e].imag(); }
    double* w = w_out.data() + (size_t)k * nr;
    auto M = [&](int i, int j) {
      std::complex<double> v = 0.0;
      for (int m = 0; m < d; ++m) v += std::conj(Kk[m * d + i]) * Kk[m * d + j];
      return v;
    };
    for (int i = 0; i < d; ++i) w[i] = M(i, i).real();
    int t = d;
    for (int i = 0; i < d; ++i) for (int j = i + 1; j < d; ++j) {
      const std::complex<double> m = M(i, j);
      w[t++] = 2.0 * m.real();
      w[t++] = -2.0 * m.imag();
    }
  }
}

// The depolarising Kraus sets of a slot without an override: sqrt(1 - p) 1, then sqrt(p / 3) X, Y, Z or
// sqrt(p / 15) P_b (x) P_a over the 15 non-identity pairs (a on q0, the low index bit; a runs fastest).
inline void qj_depol_kraus(double p, int d, std::vector<std::complex<double>>& K) {
  typedef std::complex<double> cd;
  const cd P[4][4] = {{1.0, 0.0, 0.0, 1.0}, {0.0, 1.0, 1.0, 0.0}, {0.0, cd(0.0, -1.0), cd(0.0, 1.0), 0.0}, {1.0, 0.0, 0.0, -1.0}};
  K.clear();
  if (d == 2) {
    for (int a = 0; a < 4; ++a) {
      const double s = std::sqrt(a ? p / 3.0 : 1.0 - p);
      for (int e = 0; e < 4; ++e) K.push_back(s * P[a][e]);
    }
    return;
  }
  for (int b = 0; b < 4; ++b) for (int a = 0; a < 4; ++a) {
    const double s = std::sqrt((a || b) ? p / 15.0 : 1.0 - p);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c)      // index = bit(q0) + 2 bit(q1): P_a on the low bit
      K.push_back(s * P[a][(r & 1) * 2 + (c & 1)] * P[b][(r >> 1) * 2 + (c >> 1)]);
  }
}

}  // namespace vqe

#if defined(__HIPCC__)
#include "vqe_grad.h"

namespace vqe {

static_assert(G_RX == OP_RX && G_RY == OP_RY && G_RZ == OP_RZ && G_RYY == OP_RYY, "qj_compile writes gate kinds as op kinds");
static_assert(sizeof(QjOp) == sizeof(Op), "QjOp records live in Lds::ops");

struct QjDev {
  int n1, n2;               // Kraus operators of the one- / two-qubit slot; 0: the slot is the identity
  const double* K1;         // [n1][2][2] (re, im)
  const double* W1;         // [n1][4]   weights of p_k (qj_build_tables)
  const double* K2;         // [n2][4][4] (re, im)
  const double* W2;         // [n2][16]
  int T;                    // trajectories per circuit
  uint64_t eval_id;
  const int32_t* active;    // NULL, or [batch]: 0 = the circuit's optimiser does not wait for this evaluation
  double* etraj;            // [batch * T] out
  int32_t* jumps;           // [batch * T] out: selections k != 0
  double2* state_out;       // NULL, or [2^n]: the final state of work item 0, logical order
};

constexpr size_t kQjRedBytes = 8 * 16 * 8;      // 16 partial sums of each of up to 8 waves
__host__ __device__ inline size_t qj_lds_bytes(int n, int max_ops, int max_params) {
  return ((size_t)16 << n) + (size_t)16 * max_ops + (size_t)16 * max_params + kQjRedBytes + 128 + 128 + 128 + 32;
}

// One evaluation: the trajectory launch over the batch A describes and k_qj_mean into A.fout (nfev: NULL, or [batch]
// set to 1; jsum: [batch] jumps per circuit), queued on `stream`.  Defined in vqe_qjump.hip, a translation unit - and so
// a code object - of its own: the kernels of vqe_api.hip, the fused env-step kernel among them, keep the code object
// they had before this path existed, byte for byte.  Returns 0, QJ_ETOOLARGE (the circuit does not fit the LDS),
// QJ_ESIZE (n outside 1 .. 13) or QJ_EHIP (*err); *grid: workgroups of the trajectory launch.
enum : int { QJ_OK = 0, QJ_ETOOLARGE = 1, QJ_ESIZE = 2, QJ_EHIP = 3 };
int qj_launch(const BatchArgs& A, const GradHam& GH, const QjDev& Q, int32_t* nfev, long long* jsum, int lds_per_cu,
              int cu_count, hipStream_t stream, int* grid, int* wg_per_cu, hipError_t* err);

}  // namespace vqe
#endif  // __HIPCC__

#if defined(__HIPCC__) && defined(VQE_QJUMP_KERNELS)      // (vqe_qjump.hip)
namespace vqe {

// v[j] <- the sum of v[j] over the workgroup, the same bits in every thread: DPP butterfly per wave, then the waves in
// index order.  red: NW * NR doubles; begins with a barrier when NW > 1.
template <int NW, int NR>
__device__ __forceinline__ void qj_block_sum(double (&v)[NR], double* red) {
#pragma unroll
  for (int j = 0; j < NR; ++j) v[j] = wave_sum(v[j]);
  if constexpr (NW > 1) {
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
      for (int j = 0; j < NR; ++j) red[(threadIdx.x >> 6) * NR + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += red[w * NR + j];
      v[j] = t;
    }
  }
}

// The selection rule on the reduced reals r: every thread computes the same k.  *scale = 1 / sqrt(p_k).
template <int NR>
__device__ __forceinline__ int qj_select(const double (&r)[NR], const double* __restrict__ W, int count, double u, double* scale) {
  int ksel = -1, klast = -1;
  double cum = 0.0, psel = 1.0, plast = 1.0;
  for (int k = 0; k < count; ++k) {
    double pk = 0.0;
#pragma unroll
    for (int j = 0; j < NR; ++j) pk += W[k * NR + j] * r[j];
    if (pk > 0.0) { klast = k; plast = pk; }
    cum += pk;
    if (ksel < 0 && u < cum) { ksel = k; psel = pk; }
  }
  if (ksel < 0) { ksel = klast; psel = plast; }
  if (ksel < 0) ksel = 0;                       // (no p_k > 0: not a state; K_0 is applied unscaled)
  *scale = 1.0 / sqrt(psel);
  return __builtin_amdgcn_readfirstlane(ksel);
}

__device__ __forceinline__ double2 qj_cmul(double kr, double ki, const double2& a) {
  return make_double2(kr * a.x - ki * a.y, kr * a.y + ki * a.x);
}
__device__ __forceinline__ void qj_swap(bool on, double2& a, double2& b) {
  const double2 t = a;
  if (on) { a = b; b = t; }
}

template <int N>
__global__ void __launch_bounds__(Geo<N>::NT) k_qj_traj(BatchArgs A, GradHam GH, QjDev Q) {
  constexpr int NT = Geo<N>::NT;
  constexpr int NW = Geo<N>::NW;
  constexpr uint32_t DIM = 1u << N;
  constexpr int NA = (DIM + NT - 1) / NT;       // own amplitudes per thread
  constexpr int NP = (DIM / 2 + NT - 1) / NT;   // pairs per thread
  constexpr int NQ = (DIM / 4 + NT - 1) / NT;   // quads per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x;
  unsigned char* base = smem;
  Lds L{};
  L.psi = (double2*)base; base += (size_t)16 << N;
  L.ops = (Op*)base; base += (size_t)16 * A.max_ops;
  L.cs = (double2*)base; base += (size_t)16 * A.max_params;
  double* red = (double*)base; base += kQjRedBytes;
  L.red = (double*)base; base += 128;
  L.xm = (uint32_t*)base; base += 128;
  L.zm = (uint32_t*)base; base += 128;
  L.meta = (int32_t*)base;
  L.sched = L.ops;

  const long long total = (long long)A.batch * Q.T;
  int compiled = -1;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const int b = (int)(w / Q.T), t = (int)(w % Q.T);
    if (Q.active && !Q.active[b]) continue;     // (the same for the whole workgroup)
    const int P = A.par_count[b];
    if (b != compiled) {
      // the gate records are staged in the (idle) state region when they fit there; thread 0 walks them
      const int G = A.gate_count[b];
      const GateRec* gsrc = A.gates + A.gate_begin[b];
      GateRec* gl = (GateRec*)L.psi;
      const bool staged = (uint32_t)G <= DIM;
      if (staged) for (int i = (int)tid; i < G; i += NT) ((int4*)gl)[i] = ((const int4*)gsrc)[i];
      const double* theta = A.theta + A.par_begin[b];
      for (int j = (int)tid; j < P; j += NT) {
        double s, c;
        sincos(0.5 * theta[j], &s, &c);
        L.cs[j] = make_double2(c, s);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t c = 0;
        const int nops = qj_compile(staged ? gl : gsrc, G, N, Q.n1 > 0, Q.n2 > 0, (QjOp*)L.ops, A.max_ops, L.xm, L.zm, &c);
        int permuted = (c != 0);
        for (int q = 0; q < N; ++q) if (L.xm[q] != (1u << q)) permuted = 1;
        L.meta[0] = nops <= A.max_ops ? nops : 0;      // (the host sizes max_ops by the batch: a list that does not fit is not run)
        L.meta[1] = (int32_t)c;
        L.meta[6] = permuted;
      }
      __syncthreads();
      compiled = b;
    }
    load_init<N>(L, A.init);
    __syncthreads();
    const uint64_t key = noise_key(A.noise.seed, (uint64_t)b, Q.eval_id);
    const uint64_t tsel = (uint64_t)(t + 1) << 44;
    int njump = 0;
    const int nops = L.meta[0];
    for (int o = 0; o < nops; ++o) {
      const Op op = L.ops[o];
      const int kind = op.kind & 0xff;
      const int inv = (op.kind >> 8) & 1;
      if (op_is_pair(kind)) {
        const double2 cs = L.cs[op.pidx];
        const int hb = 31 - __clz((int)op.xm);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const uint32_t q = tid + (uint32_t)k * NT;
          if (DIM / 2 >= NT || q < DIM / 2) {
            const uint32_t p0 = insert0(q, hb), p1 = p0 ^ op.xm;
            const double2 a0 = L.psi[p0], a1 = L.psi[p1];
            if (kind == OP_RX) {
              L.psi[p0] = make_double2(cs.x * a0.x - cs.y * a1.y, cs.x * a0.y + cs.y * a1.x);
              L.psi[p1] = make_double2(cs.x * a1.x - cs.y * a0.y, cs.x * a1.y + cs.y * a0.x);
            } else if (kind == OP_RY) {
              const double s0 = (parity32(p0 & op.zm) ^ inv) ? -cs.y : cs.y;
              L.psi[p0] = make_double2(cs.x * a0.x + s0 * a1.x, cs.x * a0.y + s0 * a1.y);
              L.psi[p1] = make_double2(cs.x * a1.x - s0 * a0.x, cs.x * a1.y - s0 * a0.y);
            } else {   // OP_RYY
              const double s0 = (parity32(p0 & op.zm) ^ inv) ? cs.y : -cs.y;
              L.psi[p0] = make_double2(cs.x * a0.x - s0 * a1.y, cs.x * a0.y + s0 * a1.x);
              L.psi[p1] = make_double2(cs.x * a1.x - s0 * a0.y, cs.x * a1.y + s0 * a0.x);
            }
          }
        }
      } else if (kind == OP_RZ) {
        const double2 cs = L.cs[op.pidx];
#pragma unroll
        for (int k = 0; k < NA; ++k) {
          const uint32_t p = tid + (uint32_t)k * NT;
          if (DIM >= NT || p < DIM) {
            const double s = (parity32(p & op.zm) ^ inv) ? -cs.y : cs.y;
            const double2 a = L.psi[p];
            L.psi[p] = make_double2(cs.x * a.x - s * a.y, cs.x * a.y + s * a.x);
          }
        }
      } else if (kind == QJ_JUMP1) {
        // pass 1: rho_red of the qubit.  a0 / a1: the members of the pair with the qubit at 0 / 1
        const int hb = 31 - __clz((int)op.xm);
        double r[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const uint32_t q = tid + (uint32_t)k * NT;
          if (DIM / 2 >= NT || q < DIM / 2) {
            const uint32_t p0 = insert0(q, hb);
            double2 a0 = L.psi[p0], a1 = L.psi[p0 ^ op.xm];
            qj_swap((parity32(p0 & op.zm) ^ inv) != 0, a0, a1);
            r[0] += a0.x * a0.x + a0.y * a0.y;
            r[1] += a1.x * a1.x + a1.y * a1.y;
            r[2] += a1.x * a0.x + a1.y * a0.y;
            r[3] += a1.y * a0.x - a1.x * a0.y;
          }
        }
        qj_block_sum<NW, 4>(r, red);
        double scale;
        const int ks = qj_select<4>(r, Q.W1, Q.n1, noise_uniform_k(key, tsel | (uint64_t)(uint32_t)op.pidx), &scale);
        njump += ks != 0;
        double kk[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) kk[e] = Q.K1[ks * 8 + e] * scale;
        // pass 2: psi <- K_k psi / sqrt(p_k)
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const uint32_t q = tid + (uint32_t)k * NT;
          if (DIM / 2 >= NT || q < DIM / 2) {
            const uint32_t p0 = insert0(q, hb), p1 = p0 ^ op.xm;
            const bool sw = (parity32(p0 & op.zm) ^ inv) != 0;
            double2 a0 = L.psi[p0], a1 = L.psi[p1];
            qj_swap(sw, a0, a1);
            const double2 x0 = qj_cmul(kk[0], kk[1], a0), x1 = qj_cmul(kk[2], kk[3], a1);
            const double2 y0 = qj_cmul(kk[4], kk[5], a0), y1 = qj_cmul(kk[6], kk[7], a1);
            double2 n0 = make_double2(x0.x + x1.x, x0.y + x1.y), n1 = make_double2(y0.x + y1.x, y0.y + y1.y);
            qj_swap(sw, n0, n1);
            L.psi[p0] = n0;
            L.psi[p1] = n1;
          }
        }
      } else if (kind == QJ_JUMP2) {
        const Op ob = L.ops[o + 1];               // (qj_compile writes the QJ_TAIL record together with this one)
        ++o;
        const int invb = (op.kind >> 9) & 1;
        int lo, hi;
        qj_quad_bits(op.xm, ob.xm, &lo, &hi);
        double r[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) r[j] = 0.0;
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
          const uint32_t q = tid + (uint32_t)k * NT;
          if (DIM / 4 >= NT || q < DIM / 4) {
            const uint32_t p = insert0(insert0(q, lo), hi);
            double2 v[4] = {L.psi[p], L.psi[p ^ op.xm], L.psi[p ^ ob.xm], L.psi[p ^ op.xm ^ ob.xm]};
            // v[s] is the member with local index s ^ l0, l0 that of p: order them by local index
            const bool s0 = (parity32(p & op.zm) ^ inv) != 0, s1 = (parity32(p & ob.zm) ^ invb) != 0;
            qj_swap(s0, v[0], v[1]); qj_swap(s0, v[2], v[3]);
            qj_swap(s1, v[0], v[2]); qj_swap(s1, v[1], v[3]);
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] += v[i].x * v[i].x + v[i].y * v[i].y;
            int tt = 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
              for (int j = i + 1; j < 4; ++j) {
                r[tt++] += v[j].x * v[i].x + v[j].y * v[i].y;
                r[tt++] += v[j].y * v[i].x - v[j].x * v[i].y;
              }
            }
          }
        }
        qj_block_sum<NW, 16>(r, red);
        double scale;
        const int ks = qj_select<16>(r, Q.W2, Q.n2, noise_uniform_k(key, tsel | (uint64_t)(uint32_t)op.pidx), &scale);
        njump += ks != 0;
        const double* __restrict__ Kk = Q.K2 + (size_t)ks * 32;
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
          const uint32_t q = tid + (uint32_t)k * NT;
          if (DIM / 4 >= NT || q < DIM / 4) {
            const uint32_t p = insert0(insert0(q, lo), hi);
            double2 v[4] = {L.psi[p], L.psi[p ^ op.xm], L.psi[p ^ ob.xm], L.psi[p ^ op.xm ^ ob.xm]};
            const bool s0 = (parity32(p & op.zm) ^ inv) != 0, s1 = (parity32(p & ob.zm) ^ invb) != 0;
            qj_swap(s0, v[0], v[1]); qj_swap(s0, v[2], v[3]);
            qj_swap(s1, v[0], v[2]); qj_swap(s1, v[1], v[3]);
            double2 nv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              double2 s = make_double2(0.0, 0.0);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const double2 m = qj_cmul(Kk[(i * 4 + j) * 2], Kk[(i * 4 + j) * 2 + 1], v[j]);
                s.x += m.x; s.y += m.y;
              }
              nv[i] = make_double2(s.x * scale, s.y * scale);
            }
            qj_swap(s1, nv[0], nv[2]); qj_swap(s1, nv[1], nv[3]);
            qj_swap(s0, nv[0], nv[1]); qj_swap(s0, nv[2], nv[3]);
            L.psi[p] = nv[0];
            L.psi[p ^ op.xm] = nv[1];
            L.psi[p ^ ob.xm] = nv[2];
            L.psi[p ^ op.xm ^ ob.xm] = nv[3];
          }
        }
      }
      __syncthreads();
    }
    // psi into logical order, E = <psi|H|psi>
    const int permuted = L.meta[6];
    const uint32_t coff = (uint32_t)L.meta[1];
#include "vqe_grad_energy.h"
    if (tid == 0) { Q.etraj[w] = e; Q.jumps[w] = njump; }
    if (Q.state_out && w == 0)
      for (uint32_t p = tid; p < DIM; p += NT) Q.state_out[p] = L.psi[p];
    __syncthreads();                              // the LDS is reused by the next work item
  }
}

// f[b] = the mean of the T trajectory energies in t order (+ shot noise), jsum[b] = the jumps of circuit b; one thread
// per circuit.  A circuit that is not active keeps its f and counts no jumps.
__global__ void k_qj_mean(int batch, int T, const double* __restrict__ etraj, const int32_t* __restrict__ jumps,
                          const int32_t* __restrict__ active, NoiseCfg noise, uint64_t eval_id, double* fout, int32_t* nfev,
                          long long* jsum) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= batch) return;
  if (active && !active[b]) { jsum[b] = 0; return; }
  double s = 0.0;
  long long j = 0;
  for (int t = 0; t < T; ++t) { s += etraj[(size_t)b * T + t]; j += jumps[(size_t)b * T + t]; }
  double e = s / (double)T;
  if (noise.shot_sigma != 0.0) e += noise.shot_sigma * noise_gauss(noise.seed, (uint64_t)b, eval_id);
  fout[b] = e;
  if (nfev) nfev[b] = 1;
  jsum[b] = j;
}

}  // namespace vqe
#endif  // VQE_QJUMP_KERNELS
