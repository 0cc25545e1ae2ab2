// vqe_grad.h - adjoint energy gradient of the LDS-resident path (1 <= n <= 13).
//
// One workgroup per circuit (same geometry as k_lds_energy):
//  1. forward: compile_ops (non-canonical form) + run_ops with the final gather switched off, so psi stays in the
//     physical frame of the GF(2) map;
//  2. lambda = H psi in the logical frame: psi is gathered into logical order, every thread accumulates the lambda
//     entries of its own amplitudes over all X-mask groups of this handle's shard in registers (no write conflicts),
//     E = Re <psi|lambda>; then psi and lambda are scattered back to the physical frame;
//  3. backward: for op k = K-1 .. 0 the contribution Re <lambda_k| K psi_k> (K = iP, the op at (c, s) = (0, 1); P a one- or two-qubit Pauli string) is
//     reduced per wavefront into gacc[k][wave], then U_k^-1 is applied to psi and lambda;
//  4. grad[j] = sum over the ops with parameter j (0 for a parameter no gate uses), plain stores.
// The Hamiltonian comes in its own unit-free table set (GradHam, built by the host on the first gradient request for
// a Hamiltonian): per group the pair table T[q] = D_x(p0) over p0 = insert0(q, hb(x)) in the logical index - real
// (DIM/2 doubles) or complex (DIM/2 double2) - and for the diagonal group a real table over all DIM indices.
// lambda[p0 ^ x] += T psi[p0], lambda[p0] += conj(T) psi[p0 ^ x].
// LAM_GLOBAL: lambda lives in a per-workgroup slice of a global scratch buffer (n = 13, where psi alone takes 128 KiB
// of LDS, or whenever psi + lambda + the op list do not fit beside each other); the grid is then persistent.
#pragma once
#include "vqe_device.h"

namespace vqe {

struct GradHam {
  int n_groups;
  const uint32_t* gx;       // [n_groups] X mask (logical)
  const int64_t* off;       // [n_groups] offset of the table in doubles
  const int32_t* cplx;      // [n_groups] 1: complex pair table (double2 entries)
  const double* tab;
};

__host__ __device__ inline size_t grad_lds_bytes(int n, bool lam_global, int max_ops, int max_params, int nw) {
  size_t b = (size_t)16 << n;                                  // psi
  if (!lam_global) b += (size_t)16 << n;                       // lambda
  b += (size_t)16 * max_ops + (size_t)16 * max_params;         // ops, (cos, sin)
  b += (((size_t)8 * max_ops * nw) + 15) & ~(size_t)15;        // per-wave partial gradients of every op
  return b + 128 + 128 + 128 + 32;                             // red, xm, zm, meta
}

template <int N, bool LAM_GLOBAL>
__global__ void __launch_bounds__(Geo<N>::NT) k_lds_energy_grad(BatchArgs A, GradHam GH, double* grad, double2* lam_scratch) {
  constexpr int NT = Geo<N>::NT;
  constexpr int NW = Geo<N>::NW;
  constexpr uint32_t DIM = 1u << N;
  constexpr int NA = (DIM + NT - 1) / NT;       // own amplitudes per thread
  constexpr int NP = (DIM / 2 + NT - 1) / NT;   // pairs per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x;
  const int wave = (int)(tid >> 6);
  unsigned char* base = smem;
  Lds L{};
  L.psi = (double2*)base; base += (size_t)16 << N;
  double2* lam_lds = (double2*)base;
  if (!LAM_GLOBAL) base += (size_t)16 << N;
  L.ops = (Op*)base; base += (size_t)16 * A.max_ops;
  L.cs = (double2*)base; base += (size_t)16 * A.max_params;
  double* gacc = (double*)base; base += (((size_t)8 * A.max_ops * NW) + 15) & ~(size_t)15;
  L.red = (double*)base; base += 128;
  L.xm = (uint32_t*)base; base += 128;
  L.zm = (uint32_t*)base; base += 128;
  L.meta = (int32_t*)base;
  L.sched = L.ops;

  for (int b = blockIdx.x; b < A.batch; b += gridDim.x) {
    double2* lam = LAM_GLOBAL ? lam_scratch + (size_t)blockIdx.x * DIM : lam_lds;
    const int P = A.par_count[b];
    const double* theta = A.theta + A.par_begin[b];
    // ---- 1. forward pass in the physical frame
    compile_ops(A, b, 0, L);                      // (stages the gate records in the psi region; ends with a barrier)
    const int permuted = L.meta[6];
    const uint32_t coff = (uint32_t)L.meta[1];
    load_init<N>(L, A.init);
    if (tid == 0) L.meta[3] = 0;                  // no final gather: run_ops leaves psi physical
    __syncthreads();
    run_ops<N, false>(L, theta, P);
    // physical index of logical index i: A^-1 (i ^ c)
    auto phys = [&](uint32_t i) {
      const uint32_t v = i ^ coff;
      uint32_t p = 0;
#pragma unroll
      for (int q = 0; q < N; ++q) p ^= ((v >> q) & 1u) ? L.xm[q] : 0u;
      return p;
    };
    double2 own[NA];
    if (permuted) {
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const uint32_t i = tid + (uint32_t)k * NT;
        if (DIM >= NT || i < DIM) own[k] = L.psi[phys(i)];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const uint32_t i = tid + (uint32_t)k * NT;
        if (DIM >= NT || i < DIM) L.psi[i] = own[k];
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const uint32_t i = tid + (uint32_t)k * NT;
        if (DIM >= NT || i < DIM) own[k] = L.psi[i];
      }
    }
    // ---- 2. lambda = H psi (logical frame), E = Re <psi|lambda>
    double2 acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = make_double2(0.0, 0.0);
    for (int g = 0; g < GH.n_groups; ++g) {
      const uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)GH.gx[g]);
      const double* t = GH.tab + GH.off[g];
      if (x == 0u) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
          const uint32_t i = tid + (uint32_t)k * NT;
          if (DIM >= NT || i < DIM) {
            const double d = t[i];
            acc[k].x += d * own[k].x;
            acc[k].y += d * own[k].y;
          }
        }
        continue;
      }
      const int hb = 31 - __clz((int)x);
      const bool cplx = __builtin_amdgcn_readfirstlane(GH.cplx[g]) != 0;
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const uint32_t i = tid + (uint32_t)k * NT;
        if (DIM >= NT || i < DIM) {
          const uint32_t j = i ^ x;
          const uint32_t up = (i >> hb) & 1u;            // 1: i is the p0 ^ x member of its pair
          const uint32_t i0 = up ? j : i;
          const uint32_t q = ((i0 >> (hb + 1)) << hb) | (i0 & ((1u << hb) - 1u));
          const double2 a = L.psi[j];
          if (cplx) {
            const double2 d = ((const double2*)t)[q];
            const double di = up ? d.y : -d.y;           // T for the p0 -> p0 ^ x direction, conj(T) for the other
            acc[k].x += d.x * a.x - di * a.y;
            acc[k].y += d.x * a.y + di * a.x;
          } else {
            const double d = t[q];
            acc[k].x += d * a.x;
            acc[k].y += d * a.y;
          }
        }
      }
    }
    double e_part = 0.0;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const uint32_t i = tid + (uint32_t)k * NT;
      if (DIM >= NT || i < DIM) e_part += own[k].x * acc[k].x + own[k].y * acc[k].y;
    }
    const double e = block_sum<NW>(e_part, L.red);   // (its barriers also end every read of psi above)
    __syncthreads();
    // back to the physical frame: psi[phys(i)] = psi_logical[i], the same for lambda
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const uint32_t i = tid + (uint32_t)k * NT;
      if (DIM >= NT || i < DIM) {
        const uint32_t p = permuted ? phys(i) : i;
        L.psi[p] = own[k];
        lam[p] = acc[k];
      }
    }
    __syncthreads();
    // ---- 3. backward pass
    const int nops = L.meta[0];
    for (int o = nops - 1; o >= 0; --o) {
      const Op op = L.ops[o];
      const int kind = op.kind & 0xff;
      const int inv = (op.kind >> 8) & 1;
      const double2 cs = L.cs[op.pidx];
      const double c = cs.x, s = cs.y;
      double gp = 0.0;
      if (op_is_pair(kind)) {
        const int hb = 31 - __clz((int)op.xm);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const uint32_t q = tid + (uint32_t)k * NT;
          if (DIM / 2 >= NT || q < DIM / 2) {
            const uint32_t p0 = insert0(q, hb), p1 = p0 ^ op.xm;
            const double2 a0 = L.psi[p0], a1 = L.psi[p1];
            const double2 l0 = lam[p0], l1 = lam[p1];
            if (kind == OP_RX) {
              // K = iX: (K psi)[p0] = i a1, (K psi)[p1] = i a0
              gp += l0.x * -a1.y + l0.y * a1.x + l1.x * -a0.y + l1.y * a0.x;
              // U^-1 = c I - s iX
              L.psi[p0] = make_double2(c * a0.x + s * a1.y, c * a0.y - s * a1.x);
              L.psi[p1] = make_double2(c * a1.x + s * a0.y, c * a1.y - s * a0.x);
              lam[p0] = make_double2(c * l0.x + s * l1.y, c * l0.y - s * l1.x);
              lam[p1] = make_double2(c * l1.x + s * l0.y, c * l1.y - s * l0.x);
            } else if (kind == OP_RYY) {
              const double sg = (parity32(p0 & op.zm) ^ inv) ? 1.0 : -1.0;
              // K = i sg X with one sign per pair: (K psi)[p0] = i sg a1, (K psi)[p1] = i sg a0
              gp += sg * (l0.x * -a1.y + l0.y * a1.x + l1.x * -a0.y + l1.y * a0.x);
              const double s0 = sg * s;
              L.psi[p0] = make_double2(c * a0.x + s0 * a1.y, c * a0.y - s0 * a1.x);
              L.psi[p1] = make_double2(c * a1.x + s0 * a0.y, c * a1.y - s0 * a0.x);
              lam[p0] = make_double2(c * l0.x + s0 * l1.y, c * l0.y - s0 * l1.x);
              lam[p1] = make_double2(c * l1.x + s0 * l0.y, c * l1.y - s0 * l0.x);
            } else {
              const double sg = (parity32(p0 & op.zm) ^ inv) ? -1.0 : 1.0;
              // K: (K psi)[p0] = sg a1, (K psi)[p1] = -sg a0
              gp += sg * (l0.x * a1.x + l0.y * a1.y - l1.x * a0.x - l1.y * a0.y);
              const double s0 = sg * s;
              L.psi[p0] = make_double2(c * a0.x - s0 * a1.x, c * a0.y - s0 * a1.y);
              L.psi[p1] = make_double2(c * a1.x + s0 * a0.x, c * a1.y + s0 * a0.y);
              lam[p0] = make_double2(c * l0.x - s0 * l1.x, c * l0.y - s0 * l1.y);
              lam[p1] = make_double2(c * l1.x + s0 * l0.x, c * l1.y + s0 * l0.y);
            }
          }
        }
      } else if (kind == OP_RZ) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
          const uint32_t p = tid + (uint32_t)k * NT;
          if (DIM >= NT || p < DIM) {
            const double sg = (parity32(p & op.zm) ^ inv) ? -1.0 : 1.0;
            const double2 a = L.psi[p], l = lam[p];
            // K = i sg: (K psi)[p] = sg (-a.y, a.x)
            gp += sg * (l.y * a.x - l.x * a.y);
            const double ss = sg * s;
            L.psi[p] = make_double2(c * a.x + ss * a.y, c * a.y - ss * a.x);
            lam[p] = make_double2(c * l.x + ss * l.y, c * l.y - ss * l.x);
          }
        }
      }
      gp = wave_sum(gp);
      if ((tid & 63u) == 0u) gacc[o * NW + wave] = gp;
      __syncthreads();
    }
    // ---- 4. per-parameter sums (a parameter may be shared by several gates; an unused one gets 0)
    for (int j = (int)tid; j < P; j += NT) {
      double gsum = 0.0;
      for (int o = 0; o < nops; ++o) {
        if (L.ops[o].pidx != j) continue;
#pragma unroll
        for (int w = 0; w < NW; ++w) gsum += gacc[o * NW + w];
      }
      grad[A.par_begin[b] + j] = gsum;
    }
    if (tid == 0) { A.fout[b] = e; if (A.nfev) A.nfev[b] = 1; }
    __syncthreads();                              // the LDS is reused by the next circuit of a persistent grid
  }
}

}  // namespace vqe
