// vqe_lbfgs.h - L-BFGS with Armijo backtracking on the adjoint gradient, the whole loop in one launch (1 <= n <= 13).
//
// Geometry and LDS layout of k_lds_energy_grad (vqe_grad.h): one workgroup per circuit, a persistent grid when lambda
// lives in global scratch.  compile_ops runs once per circuit (twice in an environment step: pre-action circuit, then
// the full one); every trial point costs one adjoint_eval, which only rewrites L.cs.
// The optimiser's vectors - x, g, the trial point xt, its gradient gt, the direction d and the history S[m][.], Y[m][.] -
// live in a per-workgroup slice of a global scratch buffer (rows padded to 128 bytes; a few tens of KiB, L2 resident):
// at n = 12 psi + lambda take 128 of the 160 KiB of LDS.  The per-pair scalars s.y, y.y and the alpha of the two-loop
// recursion sit in 512 bytes of LDS.  Wave 0 runs the update between two evaluations, the other waves wait at the
// barrier.  The update is lbfgs_tell below: the one device copy of the algorithm, which k_sl_step (vqe_stream_lbfgs.h)
// runs as well, one wavefront per stream, between two evaluations of the streaming path.
//
// The algorithm (tests/lbfgs_helpers.py restates it decision for decision):
//   (f, g) = eval(x0); nfev = 1; nit = 0
//   loop:  nit == maxiter -> status 4;  max|g| <= gtol -> status 0;  nfev >= maxfun -> status 3
//          d = -H g by the two-loop recursion over the stored pairs, newest first, H0 = (s.y)/(y.y) of the newest;
//          no pair: d = -g / max(1, |g|_2);  dg = g.d;  dg >= 0: drop the history, take the no-pair direction
//          t = 1; up to max_ls trials: (ft, gt) = eval(x + t d), nfev += 1;  ft <= f + c1 t dg: accept;
//                 else nfev == maxfun -> status 3;  else t *= 0.5;   no trial accepted -> status 2 (x, f unchanged)
//          s = t d, y = gt - g, stored iff s.y > 1e-10 y.y (the oldest pair leaves when m are held)
//          converged = f - ft <= ftol max(|f|, |ft|, 1);  x, f, g = x + t d, ft, gt;  nit += 1;  converged -> status 1
// Parameters whose gradient is identically 0 (used by no gate; the new gate's angle of an environment step) never move:
// every direction is a combination of gradients.
#pragma once
#include "vqe_grad.h"

namespace vqe {

struct LbfgsArgs {
  int m, maxiter, maxfun, max_ls;
  double gtol, ftol, c1;
  double* work;       // [grid][lbfgs_work_doubles(max_params, m)]
  int32_t* nit;       // [batch] accepted steps
  int32_t* status;    // [batch] LB_*
};
enum : int { LB_GTOL = 0, LB_FTOL = 1, LB_LINESEARCH = 2, LB_MAXFUN = 3, LB_MAXITER = 4 };
constexpr int kLbfgsMaxHistory = 16;

__host__ __device__ inline size_t lbfgs_row(int max_params) { return ((size_t)max_params + 15) & ~(size_t)15; }
__host__ __device__ inline size_t lbfgs_work_doubles(int max_params, int m) {
  return (5 + 2 * (size_t)m) * lbfgs_row(max_params);      // x, g, xt, gt, d, S[m], Y[m]
}
__host__ __device__ inline size_t lbfgs_lds_bytes(int n, bool lam_global, int max_ops, int max_params, int nw, int rows = -1) {
  return ((grad_lds_bytes(n, lam_global, max_ops, max_params, nw, rows) + 15) & ~(size_t)15) + 512;   // + sy, yy, alpha [16] each, control words
}

// max over the wavefront, NaN wins (a NaN gradient must not pass the gtol test)
__device__ __forceinline__ double wave_max(double v) {
  auto mx = [](double a, double o) { return (o > a || o != o) ? o : a; };
  v = mx(v, dpp_f64<0xB1>(v));
  v = mx(v, dpp_f64<0x4E>(v));
  v = mx(v, dpp_f64<0x141>(v));
  v = mx(v, dpp_f64<0x140>(v));
  return mx(mx(readlane_f64(v, 0), readlane_f64(v, 16)), mx(readlane_f64(v, 32), readlane_f64(v, 48)));
}

// What the optimiser carries from one evaluation to the next besides its vectors (in the LDS kernel: registers of wave 0).
struct LbfgsState {
  double f, t, dg;                      // value at x, step of the running line search, g.d
  int32_t ls, cnt, head, nit;           // trials of the line search, pairs held, slot of the next pair, accepted steps
  int32_t status, nfev;                 // LB_*; evaluations made (counted by the caller)
};
__host__ __device__ inline LbfgsState lbfgs_start() { return LbfgsState{0.0, 1.0, 0.0, 0, 0, 0, 0, LB_MAXITER, 0}; }

// The update between two evaluations - the one copy of the algorithm above, run by ONE WAVEFRONT (lane l owns the
// elements j = l mod 64 of every vector, so no element is ever touched by two lanes and no barrier is needed inside).
// In: e and gt, the energy and the gradient at the trial point xt; first: that evaluation was the one of x0;
// state.nfev counts it already.  x, g, d: rows of P doubles; S, Y: m rows of pitch pp; sy, yy, alpha: [kLbfgsMaxHistory] per-slot
// scalars.  Out: state advanced; xt holds the next trial point unless the optimiser stopped (then x, state.f are the
// result and state.status says why).  -> stopped
__device__ __forceinline__ bool lbfgs_tell(LbfgsState& state, const LbfgsArgs& O, int P, int m, size_t pp, double* x, double* g,
                                           double* d, double* S, double* Y, double* xt, const double* gt, double* sy,
                                           double* yy, double* alpha, double e, bool first) {
  const int lane = (int)(threadIdx.x & 63u);
  LbfgsState st = state;      // (a local, written back at the end: stores through the reference would keep the caller's state out of registers)
  auto dot = [&](const double* u, const double* v) {
    double s = 0.0;
    for (int j = lane; j < P; j += 64) s += u[j] * v[j];
    return wave_sum(s);
  };
  bool stop = false, newpoint = false;
  if (first) {
    st.f = e;
    newpoint = true;
  } else if (e <= st.f + O.c1 * st.t * st.dg) {
    double a_sy = 0.0, a_yy = 0.0;
    for (int j = lane; j < P; j += 64) {
      const double sv = st.t * d[j], yv = gt[j] - g[j];
      a_sy += sv * yv;
      a_yy += yv * yv;
    }
    a_sy = wave_sum(a_sy);
    a_yy = wave_sum(a_yy);
    if (a_sy > 1e-10 * a_yy) {       // the pair enters slot `head` (the oldest one's when m are held)
      for (int j = lane; j < P; j += 64) {
        S[(size_t)st.head * pp + j] = st.t * d[j];
        Y[(size_t)st.head * pp + j] = gt[j] - g[j];
      }
      sy[st.head] = a_sy;
      yy[st.head] = a_yy;
      st.head = st.head + 1 == m ? 0 : st.head + 1;
      st.cnt = st.cnt < m ? st.cnt + 1 : m;
    }
    const double conv = O.ftol * fmax(fmax(fabs(st.f), fabs(e)), 1.0);
    const bool converged = (st.f - e) <= conv;
    st.f = e;
    ++st.nit;
    newpoint = true;
    if (converged) { stop = true; st.status = LB_FTOL; }
  } else if (st.nfev == O.maxfun) {
    stop = true; st.status = LB_MAXFUN;
  } else if (++st.ls == O.max_ls) {
    stop = true; st.status = LB_LINESEARCH;
  } else {
    st.t *= 0.5;
  }
  if (newpoint) {
    double gmax = 0.0;
    for (int j = lane; j < P; j += 64) {
      const double gv = gt[j];
      x[j] = xt[j];
      g[j] = gv;
      const double av = fabs(gv);
      gmax = (av > gmax || av != av) ? av : gmax;
    }
    gmax = wave_max(gmax);
    if (stop) {
    } else if (st.nit >= O.maxiter) {
      stop = true; st.status = LB_MAXITER;
    } else if (gmax <= O.gtol) {
      stop = true; st.status = LB_GTOL;
    } else if (st.nfev >= O.maxfun) {
      stop = true; st.status = LB_MAXFUN;
    } else {
      bool steepest = st.cnt == 0;
      if (!steepest) {
        for (int j = lane; j < P; j += 64) d[j] = g[j];
        for (int i = 0, s = st.head; i < st.cnt; ++i) {     // newest first
          s = s == 0 ? m - 1 : s - 1;
          const double a = dot(S + (size_t)s * pp, d) / sy[s];
          alpha[s] = a;
          for (int j = lane; j < P; j += 64) d[j] -= a * Y[(size_t)s * pp + j];
        }
        const int newest = st.head == 0 ? m - 1 : st.head - 1;
        const double gamma = sy[newest] / yy[newest];
        for (int j = lane; j < P; j += 64) d[j] *= gamma;
        int s = st.head - st.cnt;
        if (s < 0) s += m;
        for (int i = 0; i < st.cnt; ++i) {                   // oldest first
          const double beta = dot(Y + (size_t)s * pp, d) / sy[s];
          const double c = alpha[s] - beta;
          for (int j = lane; j < P; j += 64) d[j] += c * S[(size_t)s * pp + j];
          s = s + 1 == m ? 0 : s + 1;
        }
        for (int j = lane; j < P; j += 64) d[j] = -d[j];
        st.dg = dot(g, d);
        if (st.dg >= 0.0) { st.cnt = 0; st.head = 0; steepest = true; }
      }
      if (steepest) {
        const double gn = sqrt(dot(g, g));
        const double den = gn > 1.0 ? gn : 1.0;
        for (int j = lane; j < P; j += 64) d[j] = -g[j] / den;
        st.dg = dot(g, d);
      }
      st.t = 1.0;
      st.ls = 0;
    }
  }
  if (!stop)
    for (int j = lane; j < P; j += 64) xt[j] = x[j] + st.t * d[j];
  state = st;
  return stop;
}

// NOISY (vqe_set_noise_grad): every trial point is the mean over the SAME T realisations (evaluation ids
// eval_base .. eval_base + T - 1, adjoint_eval_mean), a deterministic function the line search is valid on; the closing
// energy of an environment step is the single trajectory with id eval_base + T on the full circuit.  The update is untouched.
template <int N, bool LAM_GLOBAL, bool NOISY = false>
__global__ void __launch_bounds__(Geo<N>::NT) k_lds_minimize_lbfgs(BatchArgs A, GradHam GH, LbfgsArgs O, double2* lam_scratch, NoiseGrad NG) {
  constexpr int NT = Geo<N>::NT;
  constexpr int NW = Geo<N>::NW;
  constexpr uint32_t DIM = 1u << N;
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
  L.meta = (int32_t*)base; base += 32;
  L.sched = L.ops;
  base = smem + ((grad_lds_bytes(N, LAM_GLOBAL, A.max_ops, A.max_params, NW, NOISY ? NG.rows : -1) + 15) & ~(size_t)15);
  double* sy = (double*)base;                    // [16] s.y of the pair in each slot
  double* yy = sy + kLbfgsMaxHistory;            // [16] y.y
  double* alpha = yy + kLbfgsMaxHistory;         // [16] two-loop recursion
  int32_t* ctl = (int32_t*)(alpha + kLbfgsMaxHistory);      // [0] stop flag

  const int m = O.m;
  const size_t pp = lbfgs_row(A.max_params);
  double* const W = O.work + (size_t)blockIdx.x * lbfgs_work_doubles(A.max_params, m);
  double* const x = W;
  double* const g = W + pp;
  double* const xt = W + 2 * pp;
  double* const gt = W + 3 * pp;
  double* const d = W + 4 * pp;
  double* const S = W + 5 * pp;
  double* const Y = S + (size_t)m * pp;
  double2* const lam = LAM_GLOBAL ? lam_scratch + (size_t)blockIdx.x * DIM : lam_lds;

  for (int wi = blockIdx.x; wi < A.batch; wi += gridDim.x) {
    const int b = A.order[wi];
    const int P = A.par_count[b];
    const int64_t p0 = A.par_begin[b];
    const double* theta0 = A.theta + p0;
    // environment step: the optimiser sees the pre-action circuit (pre_action, vqe_geo.h); the new gate's angle stays in
    // x at its theta0 value and has gradient 0
    const PreAction pa = pre_action(A.gates + A.gate_begin[b], A.gate_count[b], A.new_gate ? A.new_gate[b] : -1);
    compile_ops(A, b, 0, L, pa.skip, NOISY, pa.skip_end);
    for (int j = (int)tid; j < P; j += NT) xt[j] = theta0[j];
    __syncthreads();
    // wave 0 only (the other waves count the evaluations and never read the rest)
    LbfgsState st = lbfgs_start();
    for (;;) {
      double e;
      if constexpr (NOISY)
        e = adjoint_eval_mean<N, LAM_GLOBAL, true>(A, GH, L, lam, gacc, xt, P, gt, b, A.noise.eval_base, NG.n_real, pa.skip, pa.skip_end);
      else
        e = adjoint_eval<N, LAM_GLOBAL, true>(A, GH, L, lam, gacc, xt, P, gt);
      ++st.nfev;
      if (pa.hole >= 0 && (int)tid == pa.hole % NT) gt[pa.hole] = 0.0;    // (the thread that stored it in adjoint_eval)
      if (A.trace && st.nfev <= A.maxfun) {   // diagnostic: the trial point (optimised parameters only) and its value
        double* tr = A.trace + ((size_t)b * A.maxfun + (size_t)(st.nfev - 1)) * (size_t)(1 + A.max_params);
        if (tid == 0) tr[0] = e;
        for (int j = (int)tid; j < P; j += NT)
          if (j != pa.hole) tr[1 + j - (pa.hole >= 0 && j > pa.hole)] = xt[j];
      }
      __syncthreads();                     // gt is complete
      if (wave == 0) {
        const bool stop = lbfgs_tell(st, O, P, m, pp, x, g, d, S, Y, xt, gt, sy, yy, alpha, e, st.nfev == 1);
        ctl[0] = stop ? 1 : 0;             // (every lane stores the same word)
      }
      __syncthreads();                     // xt, x and the stop flag are complete
      if (ctl[0]) break;
    }
    for (int j = (int)tid; j < P; j += NT) {
      const double v = x[j];
      A.xraw[p0 + j] = v;
      A.xout[p0 + j] = A.env_step ? (double)(float)v : v;
    }
    double fret = st.f;
    if (A.env_step) {
      // CircuitEnv.step: float32 round trip, then the energy of the FULL circuit (no gradient wanted)
      __syncthreads();                     // xout complete
      if constexpr (NOISY) {
        compile_ops(A, b, 0, L, -1, true);
        fret = adjoint_eval_mean<N, LAM_GLOBAL, false>(A, GH, L, lam, gacc, A.xout + p0, P, gt, b,
                                                       A.noise.eval_base + (uint64_t)NG.n_real, 1, -1, 0);
      } else {
        compile_ops(A, b, 0, L);
        fret = adjoint_eval<N, LAM_GLOBAL, false>(A, GH, L, lam, gacc, A.xout + p0, P, gt);
      }
    }
    if (tid == 0) {                        // (a thread of wave 0: st is its own)
      A.fout[b] = fret;
      A.nfev[b] = st.nfev;
      O.nit[b] = st.nit;
      O.status[b] = st.status;
    }
    __syncthreads();                       // the LDS and the scratch slice are reused by the next circuit of a persistent grid
  }
}

}  // namespace vqe
