// vqe_spsa.h - Adam-SPSA, the two-evaluation optimiser for stochastic energies, the whole loop in one launch (1 <= n <= 13).
//
// Geometry, LDS carve-up and evaluation of k_lds_minimize (vqe_device.h): one workgroup per circuit, compile_all once
// per circuit (twice in an environment step: pre-action circuit, then the full one), patch_noise per evaluation id,
// lds_evaluate, the shot-noise term.  What is gone is StagedCobyla, its resident region and its tile: the launch takes
// lds_bytes_base alone, never more than k_lds_minimize for the same (n, max_ops, max_params).
// The optimiser's vectors - x, m, v and the trial point - live in a per-workgroup slice of a global work buffer, 4 rows
// of lbfgs_row(max_params) doubles (rows padded to 128 bytes, L2 resident), as the L-BFGS keeps its vectors: at n = 12
// the state fills the LDS budget of two workgroups per CU, and one placement serves every size.
// The evaluation wants every vector register at n = 12 (two waves per SIMD, 256 VGPRs), so what the optimiser carries
// across it costs none: the scalars of the running iteration are the same on every lane and are held as scalar registers
// (spsa_uniform), and the options are read from global memory where they are used instead of living in 22 scalar
// registers of kernel arguments (with either of the two undone the compiler spills to scratch memory at n = 12).
// The update is element-wise: thread t owns the elements j = t, t + NT, ... of every row, in the trial point, in the
// update and in the (cos, sin) loop of the evaluation, so no element is ever touched by two threads; nothing is
// wave-0-only.  One barrier stands between the evaluation and the update and one behind the update.
// The algorithm is stated in spsa_m0.h (tests/spsa_helpers.py restates it); this kernel calls that header
// for the schedule scalars (once per iteration, identically on every thread) and for every element.
//
// Evaluation e of a run has id eval_base + e and trace row e: f+ of iteration k is e = 2k, f- is e = 2k + 1, and the
// closing evaluation is e = 2K - of x_K in a plain run (nfev = 2K + 1), of the FULL circuit at the float32-rounded x_K
// in an environment step (not counted: nfev = 2K, and no trace row).  K = 0 or no optimised parameter: the closing
// evaluation alone, id eval_base, nfev = 1.
#pragma once
#include "spsa_m0.h"
#include "vqe_lbfgs.h"

namespace vqe {

// a value every lane holds alike, as scalar registers
__device__ __forceinline__ double spsa_uniform(double v) { return readlane_f64(v, 0); }

struct SpsaArgs {
  const SpsaOpts* __restrict__ op;      // the options, in device memory (validated on the host: spsa_bad_option)
  double* work;                         // [batch][4 * lbfgs_row(max_params)]: x, m, v, trial point
};

__host__ __device__ inline size_t spsa_work_doubles(int max_params) { return 4 * lbfgs_row(max_params); }
__host__ __device__ inline size_t spsa_lds_bytes(int n, int max_ops, int max_params, int n_groups, int max_pair) {
  return (lds_bytes_base(n, max_ops, max_params, n_groups, max_pair) + 15) & ~(size_t)15;
}

template <int N, bool NOISY>
__global__ void __launch_bounds__(Geo<N>::NT, Geo<N>::WPS) k_lds_minimize_spsa(BatchArgs A, SpsaArgs S) {
  constexpr int kThreads = Geo<N>::NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds L = carve(smem, N, A.max_ops, A.max_params, A.ham.n_groups, A.max_pair);
  const int tid = (int)threadIdx.x;
  const int b = A.order[blockIdx.x];
  const int P = A.par_count[b];
  const int64_t p0 = A.par_begin[b];
  const double* theta0 = A.theta + p0;
  // environment step: the optimiser sees the pre-action circuit (pre_action, vqe_geo.h); the new gate's angle stays in
  // x at its theta0 value (its perturbation sign is 0)
  const PreAction pa = pre_action(A.gates + A.gate_begin[b], A.gate_count[b], A.new_gate ? A.new_gate[b] : -1);
  const int Popt = P - (pa.hole >= 0);
  const int K = Popt > 0 ? S.op->maxiter : 0;
  const size_t pp = lbfgs_row(A.max_params);
  double* const W = S.work + (size_t)blockIdx.x * spsa_work_doubles(A.max_params);
  double* const x = W;
  double* const m = W + pp;
  double* const v = W + 2 * pp;
  double* const xt = W + 3 * pp;

  stage_groups(A.ham, L);
  if constexpr (N >= 10) stage_cls<N>(A.ham, L);
  for (int j = tid; j < P; j += kThreads) {
    x[j] = theta0[j];
    m[j] = 0.0;
    v[j] = 0.0;
  }
  SpsaIter it = spsa_start();
  double fp = 0.0;
  double fret = 0.0;
  bool need_compile = true;
  const auto sign_of = [&](uint64_t key, int j) {
    return j == pa.hole ? 0.0 : (noise_uniform_k(key, (uint64_t)j) < 0.5 ? 1.0 : -1.0);
  };
  // ONE evaluation call site keeps everything inlined once
  for (int e = 0; e <= 2 * K; ++e) {
    const bool closing = e == 2 * K;
    const bool full = closing && A.env_step;      // the full circuit at the rounded optimum
    const double* th = x;
    if (!closing) {
      if (!(e & 1)) {      // the schedule of iteration k: once, identically on every thread
        spsa_begin_iteration(it, *S.op, e >> 1);
        it.a_k = spsa_uniform(it.a_k); it.c_k = spsa_uniform(it.c_k); it.b1k = spsa_uniform(it.b1k);
      }
      const double c_k = it.c_k;
      const uint64_t key = noise_key(S.op->seed, (uint64_t)b, (uint64_t)(e >> 1));
      const double step = (e & 1) ? -c_k : c_k;
      for (int j = tid; j < P; j += kThreads) xt[j] = x[j] + step * sign_of(key, j);
      th = xt;
    } else {
      for (int j = tid; j < P; j += kThreads) {
        const double xv = x[j];
        A.xraw[p0 + j] = xv;
        A.xout[p0 + j] = A.env_step ? (double)(float)xv : xv;
      }
      if (full) { th = A.xout + p0; need_compile = need_compile || pa.skip >= 0; }
    }
    __syncthreads();                       // the point of this evaluation is complete
    const int sk = full ? -1 : pa.skip;
    const int ske = full ? 0 : pa.skip_end;
    const uint64_t eid = A.noise.eval_base + (uint64_t)e;
    if (need_compile) { compile_all<N>(A, b, 0, L, sk, true, NOISY, ske); need_compile = false; }
    if constexpr (NOISY) patch_noise<N>(A, b, eid, L, sk, true, ske);
    double f = lds_evaluate<N, NOISY>(A, L, th, P);
    // finite-shot estimate of <H>: Gaussian with the total standard deviation the caller set
    if (A.noise.shot_sigma != 0.0) f += A.noise.shot_sigma * noise_gauss(A.noise.seed, (uint64_t)b, eid);
    if (A.trace && !(full && K > 0)) {     // diagnostic: the point (optimised parameters only) and its value
      double* tr = A.trace + ((size_t)b * A.maxfun + (size_t)e) * (size_t)(1 + A.max_params);
      if (tid == 0) tr[0] = f;
      for (int j = tid; j < P; j += kThreads)
        if (j != pa.hole) tr[1 + j - (pa.hole >= 0 && j > pa.hole)] = th[j];
    }
    if (closing) {
      fret = f;
    } else if (!(e & 1)) {
      fp = spsa_uniform(f);
    } else {
      spsa_close_iteration(it, *S.op, fp, f);
      it.b1p = spsa_uniform(it.b1p); it.b2p = spsa_uniform(it.b2p);
      const uint64_t key = noise_key(S.op->seed, (uint64_t)b, (uint64_t)(e >> 1));
      __syncthreads();                     // the evaluation has read its point
      for (int j = tid; j < P; j += kThreads) {
        double xv = x[j], mv = m[j], vv = v[j];
        spsa_update_element(it, *S.op, sign_of(key, j), xv, mv, vv);
        x[j] = xv;
        m[j] = mv;
        v[j] = vv;
      }
      __syncthreads();                     // x, m, v are those of the next iteration
    }
  }
  if (tid == 0) {
    A.fout[b] = fret;
    A.nfev[b] = (A.env_step && K > 0) ? 2 * K : 2 * K + 1;
  }
}

}  // namespace vqe
