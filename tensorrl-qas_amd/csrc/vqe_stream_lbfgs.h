// vqe_stream_lbfgs.h - the device L-BFGS of vqe_lbfgs.h on the HBM-streaming path (n >= 14, opt-in by
// vqe_set_stream_lbfgs), DESIGN 4.11.
//
// The algorithm is the one at the head of vqe_lbfgs.h, decision for decision.  There one launch holds the whole loop and
// wave 0 runs the update between two adjoint_eval calls; here an evaluation is a train of launches over states in HBM
// (stream_energy_grad, vqe_stream_grad.h), so the loop is cut at the evaluation: all resident streams are evaluated in
// lock-step, and between two evaluations k_sl_step - one WAVEFRONT per stream - takes ("tells") the energy and the
// gradient just computed and leaves the next trial point where the next evaluation reads its angles.  The host only
// queues launches (vqe_api.hip: stream_lbfgs), as it does for k_s_cobyla.
//
// Lane l owns the elements j = l mod 64 of every vector, so no element is ever touched by two lanes and the update needs
// no barrier; dot products by wave_sum, max|g| by wave_max, every sum in the order of the LDS kernel.
// The vectors x, g, d, S[m], Y[m] of a stream live in its slice of the work buffer (the rows of lbfgs_work_doubles; the
// rows xt and gt of that layout stay unused: the trial point lives in the evaluation's theta buffer, its gradient in
// the gradient buffer).  What wave 0 of the LDS kernel carries in registers from one evaluation to the next, with
// s.y and y.y of the stored pairs and the running flag, is the stream's StreamLbfgsRec, loaded at entry and stored at
// exit.
// A stream that stops writes x, f, nfev, nit and status to the result arrays and clears its flag; its trial point
// stays where it is (the evaluations go on over all streams) and nothing of it is written again.
#pragma once
#include "vqe_lbfgs.h"

namespace vqe {

struct StreamLbfgsRec {
  double f, t, dg;                      // value at x, step of the running line search, g.d
  int32_t ls, cnt, head, nit;           // trials of the line search, pairs held, slot of the next pair, accepted steps
  int32_t status, nfev, active, pad_;
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
  double* const sy = R->sy;
  double* const yy = R->yy;
  auto dot = [&](const double* u, const double* v) {
    double s = 0.0;
    for (int j = lane; j < P; j += 64) s += u[j] * v[j];
    return wave_sum(s);
  };
  double f = 0.0, t = 1.0, dg = 0.0;
  int ls = 0, cnt = 0, head = 0, nit = 0, status = LB_MAXITER, nfev = 0;
  if (!FIRST) {
    f = R->f; t = R->t; dg = R->dg;
    ls = R->ls; cnt = R->cnt; head = R->head; nit = R->nit; status = R->status; nfev = R->nfev;
  }
  const double e = T.f[b];
  ++nfev;
  bool stop = false, newpoint = false;
  if (FIRST) {
    f = e;
    newpoint = true;
  } else if (e <= f + O.c1 * t * dg) {
    double a_sy = 0.0, a_yy = 0.0;
    for (int j = lane; j < P; j += 64) {
      const double sv = t * d[j], yv = gt[j] - g[j];
      a_sy += sv * yv;
      a_yy += yv * yv;
    }
    a_sy = wave_sum(a_sy);
    a_yy = wave_sum(a_yy);
    if (a_sy > 1e-10 * a_yy) {       // the pair enters slot `head` (the oldest one's when m are held)
      for (int j = lane; j < P; j += 64) {
        S[(size_t)head * pp + j] = t * d[j];
        Y[(size_t)head * pp + j] = gt[j] - g[j];
      }
      sy[head] = a_sy;
      yy[head] = a_yy;
      head = head + 1 == m ? 0 : head + 1;
      cnt = cnt < m ? cnt + 1 : m;
    }
    const double conv = O.ftol * fmax(fmax(fabs(f), fabs(e)), 1.0);
    const bool converged = (f - e) <= conv;
    f = e;
    ++nit;
    newpoint = true;
    if (converged) { stop = true; status = LB_FTOL; }
  } else if (nfev == O.maxfun) {
    stop = true; status = LB_MAXFUN;
  } else if (++ls == O.max_ls) {
    stop = true; status = LB_LINESEARCH;
  } else {
    t *= 0.5;
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
    } else if (nit >= O.maxiter) {
      stop = true; status = LB_MAXITER;
    } else if (gmax <= O.gtol) {
      stop = true; status = LB_GTOL;
    } else if (nfev >= O.maxfun) {
      stop = true; status = LB_MAXFUN;
    } else {
      bool steepest = cnt == 0;
      if (!steepest) {
        for (int j = lane; j < P; j += 64) d[j] = g[j];
        for (int i = 0, s = head; i < cnt; ++i) {           // newest first
          s = s == 0 ? m - 1 : s - 1;
          const double a = dot(S + (size_t)s * pp, d) / sy[s];
          alpha[s] = a;
          for (int j = lane; j < P; j += 64) d[j] -= a * Y[(size_t)s * pp + j];
        }
        const int newest = head == 0 ? m - 1 : head - 1;
        const double gamma = sy[newest] / yy[newest];
        for (int j = lane; j < P; j += 64) d[j] *= gamma;
        int s = head - cnt;
        if (s < 0) s += m;
        for (int i = 0; i < cnt; ++i) {                      // oldest first
          const double beta = dot(Y + (size_t)s * pp, d) / sy[s];
          const double c = alpha[s] - beta;
          for (int j = lane; j < P; j += 64) d[j] += c * S[(size_t)s * pp + j];
          s = s + 1 == m ? 0 : s + 1;
        }
        for (int j = lane; j < P; j += 64) d[j] = -d[j];
        dg = dot(g, d);
        if (dg >= 0.0) { cnt = 0; head = 0; steepest = true; }
      }
      if (steepest) {
        const double gn = sqrt(dot(g, g));
        const double den = gn > 1.0 ? gn : 1.0;
        for (int j = lane; j < P; j += 64) d[j] = -g[j] / den;
        dg = dot(g, d);
      }
      t = 1.0;
      ls = 0;
    }
  }
  if (!stop) {
    for (int j = lane; j < P; j += 64) xt[j] = x[j] + t * d[j];
  } else {
    for (int j = lane; j < P; j += 64) T.xres[p0 + j] = x[j];
  }
  if (lane == 0) {
    R->f = f; R->t = t; R->dg = dg;
    R->ls = ls; R->cnt = cnt; R->head = head; R->nit = nit; R->status = status; R->nfev = nfev;
    R->active = stop ? 0 : 1;
    if (stop) {
      T.fres[b] = f;
      T.nfres[b] = nfev;
      O.nit[b] = nit;
      O.status[b] = status;
    } else {
      atomicAdd(T.n_active, 1);
    }
  }
}

}  // namespace vqe
