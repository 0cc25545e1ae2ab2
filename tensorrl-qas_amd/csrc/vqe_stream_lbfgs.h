// vqe_stream_lbfgs.h - the device L-BFGS of vqe_lbfgs.h on the HBM-streaming path (n >= 14, opt-in by
// vqe_set_stream_lbfgs), DESIGN 4.11.
//
// The algorithm is the one at the head of vqe_lbfgs.h, and the update is that header's lbfgs_tell itself.  There one
// launch holds the whole loop and wave 0 runs the update between two adjoint_eval calls; here an evaluation is a train of
// launches over states in HBM (stream_energy_grad, vqe_stream_grad.h), so the loop is cut at the evaluation: all resident
// streams are evaluated in lock-step, and between two evaluations k_sl_step - one WAVEFRONT per stream - takes ("tells")
// the energy and the gradient just computed and leaves the next trial point where the next evaluation reads its angles.
// The host only queues launches (vqe_api.hip: lockstep_run), as it does for k_s_cobyla.
//
// The vectors x, g, d, S[m], Y[m] of a stream live in its slice of the work buffer (the rows of lbfgs_work_doubles; the
// rows xt and gt of that layout stay unused: the trial point lives in the evaluation's theta buffer, its gradient in
// the gradient buffer).  What wave 0 of the LDS kernel carries in registers from one evaluation to the next (LbfgsState),
// with s.y and y.y of the stored pairs and the running flag, is the stream's StreamLbfgsRec, loaded at entry and stored
// at exit.
// A stream that stops writes x, f, nfev, nit and status to the result arrays and clears its flag; its trial point
// stays where it is (the evaluations go on over all streams) and nothing of it is written again.
#pragma once
#include "vqe_lbfgs.h"

namespace vqe {

struct StreamLbfgsRec {
  LbfgsState st;
  int32_t active, pad_;
  double sy[kLbfgsMaxHistory], yy[kLbfgsMaxHistory];      // s.y and y.y of the pair in each slot
};

struct StreamLbfgsArgs {
  const int64_t* pbeg;       // [batch] layout of theta, grad and xres
  const int32_t* pcnt;
  int max_params;            // rows of the work buffer are lbfgs_row(max_params) doubles
  StreamLbfgsRec* rec;       // [batch]
  double* xtrial;            // in: the point just evaluated; out: the next trial point (running streams only)
  const double* f;           // [batch] energy at xtrial
  const double* grad;        // gradient at xtrial
  int32_t* n_active;         // += 1 per stream that wants another evaluation
  double* xres;              // results of the streams that stopped
  double* fres;
  int32_t* nfres;
};

// FIRST: the evaluation of x0 (xtrial holds x0).  Else: the evaluation of the trial point the previous step left.
template <bool FIRST>
__global__ void __launch_bounds__(64) k_sl_step(StreamLbfgsArgs T, LbfgsArgs O) {
  __shared__ double alpha[kLbfgsMaxHistory];      // two-loop recursion (every lane stores the same value)
  const int b = (int)blockIdx.x;
  const int lane = (int)threadIdx.x;
  StreamLbfgsRec* const R = T.rec + b;
  if (!FIRST && !R->active) return;               // (wave-uniform)
  const int P = T.pcnt[b];
  const int64_t p0 = T.pbeg[b];
  const int m = O.m;
  const size_t pp = lbfgs_row(T.max_params);
  double* const W = O.work + (size_t)b * lbfgs_work_doubles(T.max_params, m);
  double* const x = W;
  double* const g = W + pp;
  double* const d = W + 4 * pp;
  double* const S = W + 5 * pp;
  double* const Y = S + (size_t)m * pp;
  double* const xt = T.xtrial + p0;
  const double* const gt = T.grad + p0;
  LbfgsState st = FIRST ? lbfgs_start() : R->st;
  ++st.nfev;
  const bool stop = lbfgs_tell(st, O, P, m, pp, x, g, d, S, Y, xt, gt, R->sy, R->yy, alpha, T.f[b], FIRST);
  if (lane == 0) R->st = st;
  if (!stop) {
    if (lane == 0) { R->active = 1; atomicAdd(T.n_active, 1); }
    return;
  }
  for (int j = lane; j < P; j += 64) T.xres[p0 + j] = x[j];
  if (lane == 0) {
    R->active = 0;
    T.fres[b] = st.f;
    T.nfres[b] = st.nfev;
    O.nit[b] = st.nit;
    O.status[b] = st.status;
  }
}

}  // namespace vqe
