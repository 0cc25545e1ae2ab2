// vqe_grad.h - adjoint energy gradient of the LDS-resident path (1 <= n <= 13).
//
// One workgroup per circuit (same geometry as k_lds_energy).  Steps 1 (after compile_ops) to 4 are the text of
// vqe_grad_body.h, expanded in k_lds_energy_grad and in the device function adjoint_eval, which k_lds_minimize_lbfgs
// (vqe_lbfgs.h) calls once per trial point:
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
// NOISY (vqe_set_noise_grad): the mean over T frozen Pauli-noise realisations.  The ops are compiled once
// per circuit with their noise slots (compile_ops, slots = true); the workgroup then loops over t = 0 .. T-1: the patch
// of evaluation id eval_base + t (patch_noise<N, true>, the draws of the energy path), the body above, E and the
// per-parameter sums added in ascending t and divided once.  The noiseless instances carry none of this.
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

// What the NOISY instances take beside the arguments of the noiseless ones: T, and the rows of gacc - the largest number
// of ops WITH a parameter in a circuit of the batch (the noise slots take none).  rows < 0: noiseless, a row per op.
struct NoiseGrad { int n_real, rows; };

__host__ __device__ inline size_t grad_lds_bytes(int n, bool lam_global, int max_ops, int max_params, int nw, int rows = -1) {
  size_t b = (size_t)16 << n;                                  // psi
  if (!lam_global) b += (size_t)16 << n;                       // lambda
  b += (size_t)16 * max_ops + (size_t)16 * max_params;         // ops, (cos, sin)
  b += (((size_t)8 * (rows < 0 ? max_ops : rows) * nw) + 15) & ~(size_t)15;   // per-wave partial gradients of every op
  return b + 128 + 128 + 128 + 32;                             // red, xm, zm, meta
}

// One evaluation with the ops already compiled (compile_ops; only L.cs changes between two evaluations of a circuit):
// forward sweep at theta[0..P), lambda = H psi, and - BACKWARD - the backward sweep and the per-parameter sums into
// gdst[0..P).  Returns E in every thread.  k_lds_minimize_lbfgs (vqe_lbfgs.h) calls it once per trial point; its body is
// vqe_grad_body.h, the text k_lds_energy_grad expands in place (see there for why that kernel does not call this).
// NOISY: ONE realisation - the ops carry its patch; nz_t of nz_T as vqe_grad_body.h states (adjoint_eval_mean loops).
template <int N, bool LAM_GLOBAL, bool BACKWARD = true, bool NOISY = false>
__device__ __forceinline__ double adjoint_eval(const BatchArgs& A, const GradHam& GH, const Lds& L, double2* lam, double* gacc,
                                               const double* theta, int P, double* gdst, int nz_t = 0, int nz_T = 1) {
  constexpr int NT = Geo<N>::NT;
  constexpr int NW = Geo<N>::NW;
  constexpr uint32_t DIM = 1u << N;
  constexpr int NA = (DIM + NT - 1) / NT;       // own amplitudes per thread
  constexpr int NP = (DIM / 2 + NT - 1) / NT;   // pairs per thread
  const uint32_t tid = threadIdx.x;
  const int wave = (int)(tid >> 6);
#define ADJOINT_GRAD_DST(j) gdst[j]
#include "vqe_grad_body.h"
#undef ADJOINT_GRAD_DST
  return e;
}

// E_T and its gradient at theta: the mean over the realisations with evaluation ids id0 .. id0 + T - 1 of circuit b, whose
// ops were compiled with slots and without the gates [skip, skip_end).  Every thread must have left the previous reader of
// L.ops behind (the patch rewrites them): the barrier in front of the patch sees to it.
template <int N, bool LAM_GLOBAL, bool BACKWARD = true>
__device__ __forceinline__ double adjoint_eval_mean(const BatchArgs& A, const GradHam& GH, const Lds& L, double2* lam, double* gacc,
                                                    const double* theta, int P, double* gdst, int b, uint64_t id0, int T, int skip,
                                                    int skip_end) {
  double esum = 0.0;
  for (int t = 0; t < T; ++t) {
    __syncthreads();
    patch_noise<N, true>(A, b, id0 + (uint64_t)t, L, skip, false, skip_end);
    esum += adjoint_eval<N, LAM_GLOBAL, BACKWARD, true>(A, GH, L, lam, gacc, theta, P, gdst, t, T);
  }
  return esum / (double)T;
}

template <int N, bool LAM_GLOBAL, bool NOISY = false>
__global__ void __launch_bounds__(Geo<N>::NT) k_lds_energy_grad(BatchArgs A, GradHam GH, double* grad, double2* lam_scratch, NoiseGrad NG) {
  constexpr int NT = Geo<N>::NT;
  constexpr int NW = Geo<N>::NW;
  constexpr uint32_t DIM = 1u << N;
  constexpr int NA = (DIM + NT - 1) / NT;       // own amplitudes per thread
  constexpr int NP = (DIM / 2 + NT - 1) / NT;   // pairs per thread
  constexpr bool BACKWARD = true;
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
  double* gacc = (double*)base; base += (((size_t)8 * (NOISY ? NG.rows : A.max_ops) * NW) + 15) & ~(size_t)15;
  L.red = (double*)base; base += 128;
  L.xm = (uint32_t*)base; base += 128;
  L.zm = (uint32_t*)base; base += 128;
  L.meta = (int32_t*)base;
  L.sched = L.ops;

  for (int b = blockIdx.x; b < A.batch; b += gridDim.x) {
    double2* lam = LAM_GLOBAL ? lam_scratch + (size_t)blockIdx.x * DIM : lam_lds;
    const int P = A.par_count[b];
    const double* theta = A.theta + A.par_begin[b];
    if constexpr (NOISY) {
      compile_ops(A, b, 0, L, -1, true);
      // (a call here: the noisy instance is bound by its T sweeps, not by the registers of <13, true>)
      const double e = adjoint_eval_mean<N, LAM_GLOBAL>(A, GH, L, lam, gacc, theta, P, grad + A.par_begin[b], b,
                                                        A.noise.eval_base, NG.n_real, -1, 0);
      if (tid == 0) { A.fout[b] = e; if (A.nfev) A.nfev[b] = 1; }
    } else {
    constexpr int nz_t = 0, nz_T = 1;             // (names of the NOISY text of the body, which this branch discards)
    compile_ops(A, b, 0, L);                      // (stages the gate records in the psi region; ends with a barrier)
#define ADJOINT_GRAD_DST(j) grad[A.par_begin[b] + j]
#include "vqe_grad_body.h"
#undef ADJOINT_GRAD_DST
    if (tid == 0) { A.fout[b] = e; if (A.nfev) A.nfev[b] = 1; }
    }
    __syncthreads();                              // the LDS is reused by the next circuit of a persistent grid
  }
}

}  // namespace vqe
