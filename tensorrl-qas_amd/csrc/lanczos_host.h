// lanczos_host.h - host logic of the device Lanczos solver (vqe_lanczos, csrc/vqe_lanczos.h).
// Host only, no HIP: tests/cpp/lanczos_host_check.cpp compiles it with g++ and holds it without a GPU.
//   lz_tridiag_extreme  the lowest or highest eigenpair of the symmetric tridiagonal T the recurrence builds
//                       (bisection on the Sturm count, then inverse iteration; no LAPACK);
//   lz_decide           the stop rule, a pure function of (alpha, beta, options, counters);
//   lz_basis_capacity   how many basis vectors the solver keeps.
// Several eigenpairs (vqe_lanczos_multi: thick restart, locking by deflation, one stage per pair):
//   lz_sym_eig          all eigenpairs of a dense symmetric matrix - the projected matrix after a thick restart is a
//                       diagonal bordered by one row and a tridiagonal tail (Householder tridiagonalisation, implicit QL);
//   lz_keep_count       how many Ritz vectors a thick restart keeps;
//   lz_multi_slots, lz_stage_capacity   the storage rule: locked vectors in slots 0 .. e-1, the active basis behind them;
//   LzMulti             the stage / look / restart / lock state machine: "what to queue next" from alpha, beta, the
//                       breakdown flag and the options.  Whoever executes its commands (the device driver lz_run_multi of
//                       vqe_lanczos.h, or plain loops on a dense matrix in tests/cpp/lanczos_multi_host_check.cpp) owns
//                       the vectors; the machine sees O(basis) doubles per look.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace vqe {

// eigenvalues of T (diagonal alpha[0..m), off-diagonal beta[0..m-1)) that lie below x: the negative pivots of the LDL^T
// factorisation of T - x
inline int lz_sturm_count(const double* alpha, const double* beta, int m, double x, double pivmin) {
  int count = 0;
  double d = 1.0;
  for (int i = 0; i < m; ++i) {
    const double b = i ? beta[i - 1] : 0.0;
    d = (alpha[i] - x) - (i ? b * b / d : 0.0);
    if (std::fabs(d) < pivmin) d = -pivmin;
    if (d < 0.0) ++count;
  }
  return count;
}

// The extreme eigenpair of the m x m symmetric tridiagonal with diagonal alpha[0..m) and off-diagonal beta[0..m-1):
// which = 0 the lowest, 1 the highest.  theta by bisection until the interval cannot shrink (a few ulp of |T|), s[0..m)
// by inverse iteration on T - theta (Gaussian elimination with partial pivoting), |s| = 1, largest component positive.
// Returns false for m < 1.
inline bool lz_tridiag_extreme(const double* alpha, const double* beta, int m, int which, double* theta, double* s) {
  if (m < 1 || !alpha || !theta) return false;
  if (m == 1) {
    *theta = alpha[0];
    if (s) s[0] = 1.0;
    return true;
  }
  double lo = std::numeric_limits<double>::infinity(), hi = -lo, tnorm = 0.0;
  for (int i = 0; i < m; ++i) {
    const double r = (i ? std::fabs(beta[i - 1]) : 0.0) + (i + 1 < m ? std::fabs(beta[i]) : 0.0);
    lo = std::min(lo, alpha[i] - r);
    hi = std::max(hi, alpha[i] + r);
    tnorm = std::max(tnorm, std::fabs(alpha[i]) + r);
  }
  const double eps = std::numeric_limits<double>::epsilon();
  const double pivmin = std::max(tnorm * eps * eps, std::numeric_limits<double>::min());
  lo -= 2.0 * eps * tnorm + pivmin;
  hi += 2.0 * eps * tnorm + pivmin;
  // the wanted eigenvalue is the only one in (lo, hi] with count(hi) - count(lo) crossing `want`
  const int want = which ? m - 1 : 0;      // eigenvalues strictly below the wanted one
  for (int it = 0; it < 2000; ++it) {
    const double mid = lo + 0.5 * (hi - lo);
    if (!(mid > lo && mid < hi)) break;
    if (lz_sturm_count(alpha, beta, m, mid, pivmin) > want) hi = mid; else lo = mid;
  }
  const double th = lo + 0.5 * (hi - lo);
  *theta = th;
  if (!s) return true;
  // inverse iteration: (T - th) = P L U once, then a few solves from a start with no zero component
  std::vector<double> du(m), dd(m), du2(m), l(m), rhs(m);
  std::vector<char> swapped(m);
  for (int i = 0; i < m; ++i) { dd[i] = alpha[i] - th; du[i] = i + 1 < m ? beta[i] : 0.0; du2[i] = 0.0; }
  const double tiny = std::max(eps * tnorm, std::numeric_limits<double>::min());
  for (int i = 0; i + 1 < m; ++i) {
    const double sub = beta[i];
    if (std::fabs(dd[i]) >= std::fabs(sub)) {      // no row exchange
      if (dd[i] == 0.0) dd[i] = tiny;
      l[i] = sub / dd[i];
      swapped[i] = 0;
      dd[i + 1] -= l[i] * du[i];
    } else {                                       // rows i and i + 1 change places
      l[i] = dd[i] / sub;
      swapped[i] = 1;
      const double d1 = dd[i + 1], u1 = du[i];
      dd[i] = sub;
      du[i] = d1;
      du2[i] = i + 2 < m ? du[i + 1] : 0.0;
      dd[i + 1] = u1 - l[i] * d1;
      if (i + 2 < m) du[i + 1] = -l[i] * du2[i];
    }
  }
  if (std::fabs(dd[m - 1]) < tiny) dd[m - 1] = dd[m - 1] < 0.0 ? -tiny : tiny;
  for (int i = 0; i < m; ++i) s[i] = 1.0 / std::sqrt((double)m) * ((i & 1) ? 0.75 : 1.0);
  double best = std::numeric_limits<double>::infinity();
  std::vector<double> x(m);
  for (int it = 0; it < 6; ++it) {
    for (int i = 0; i < m; ++i) x[i] = s[i];
    for (int i = 0; i + 1 < m; ++i) {              // forward: L^-1 P
      if (swapped[i]) std::swap(x[i], x[i + 1]);
      x[i + 1] -= l[i] * x[i];
    }
    for (int i = m - 1; i >= 0; --i) {             // back substitution with U (three diagonals)
      double v = x[i];
      if (i + 1 < m) v -= du[i] * x[i + 1];
      if (i + 2 < m) v -= du2[i] * x[i + 2];
      double p = dd[i];
      if (std::fabs(p) < tiny) p = p < 0.0 ? -tiny : tiny;
      x[i] = v / p;
    }
    double scale = 0.0;
    for (int i = 0; i < m; ++i) scale = std::max(scale, std::fabs(x[i]));
    if (!(scale > 0.0) || !std::isfinite(scale)) break;
    double nrm = 0.0;
    for (int i = 0; i < m; ++i) { x[i] /= scale; nrm += x[i] * x[i]; }
    nrm = std::sqrt(nrm);
    for (int i = 0; i < m; ++i) x[i] /= nrm;
    double res = 0.0;                               // |T x - th x|
    for (int i = 0; i < m; ++i) {
      double v = (alpha[i] - th) * x[i];
      if (i) v += beta[i - 1] * x[i - 1];
      if (i + 1 < m) v += beta[i] * x[i + 1];
      res += v * v;
    }
    res = std::sqrt(res);
    if (res < best) {
      best = res;
      for (int i = 0; i < m; ++i) s[i] = x[i];
    } else {
      break;                                        // no further gain: keep the best iterate
    }
    if (best <= 4.0 * eps * tnorm) break;
  }
  int big = 0;
  for (int i = 1; i < m; ++i) if (std::fabs(s[i]) > std::fabs(s[big])) big = i;
  if (s[big] < 0.0) for (int i = 0; i < m; ++i) s[i] = -s[i];
  return true;
}

enum LzDecision { LZ_CONTINUE = 0, LZ_CONVERGED = 1, LZ_RESTART = 2, LZ_BREAKDOWN = 3, LZ_BUDGET = 4 };

struct LzRule {
  int which;        // 0 lowest, 1 highest
  int capacity;     // basis vectors the solver keeps
  int max_matvec;   // H applications of the recurrence, all cycles together
  double tol;
};
struct LzCounters {
  int steps;        // Lanczos steps of the current cycle whose alpha and beta are in the arrays
  int matvecs;      // H applications made so far, all cycles together
  int broke;        // -1, or the step of the current cycle at which beta was negligible (the device flag)
};

// The stop rule after `steps` steps of a cycle.  theta and s[0..*dim) receive the extreme Ritz pair of T_dim, where
// dim = broke + 1 at a breakdown (the invariant subspace) and steps otherwise.  In this order:
//   breakdown  the device flag is set;
//   converged  |beta[dim-1] * s[dim-1]| <= tol * max(1, |theta|) - in exact arithmetic the residual of the Ritz pair;
//   budget     max_matvec applications are used up;
//   restart    the basis is full;
//   continue   otherwise.
inline int lz_decide(const double* alpha, const double* beta, const LzRule& rule, const LzCounters& c, double* theta,
                     double* s, int* dim) {
  const int k = c.broke >= 0 ? c.broke + 1 : c.steps;
  *dim = k;
  if (k < 1) return c.matvecs >= rule.max_matvec ? LZ_BUDGET : LZ_CONTINUE;
  lz_tridiag_extreme(alpha, beta, k, rule.which, theta, s);
  if (c.broke >= 0) return LZ_BREAKDOWN;
  if (std::fabs(beta[k - 1] * s[k - 1]) <= rule.tol * std::max(1.0, std::fabs(*theta))) return LZ_CONVERGED;
  if (c.matvecs >= rule.max_matvec) return LZ_BUDGET;
  if (k >= rule.capacity) return LZ_RESTART;
  return LZ_CONTINUE;
}

constexpr int kLzWorkVectors = 3;      // w, the Ritz vector y, H y

// Basis vectors the solver keeps: min(max_basis, 2^n, what `budget_bytes` holds beside the three work vectors), each
// vector 2^n complex128.  Below 2 there is no recurrence: the caller answers VQE_ENOMEM.
inline int lz_basis_capacity(uint64_t budget_bytes, int n, int max_basis) {
  const uint64_t vec = (uint64_t)16 << n;
  const uint64_t fit = budget_bytes / vec;
  const uint64_t room = fit > (uint64_t)kLzWorkVectors ? fit - kLzWorkVectors : 0;
  uint64_t cap = std::min<uint64_t>(room, (uint64_t)1 << n);
  cap = std::min<uint64_t>(cap, max_basis > 0 ? (uint64_t)max_basis : 0);
  return (int)cap;
}

// ---- several eigenpairs ---------------------------------------------------------------------------------------------------

// All eigenpairs of the symmetric n x n matrix a (row major; only read).  w[0..n) ascending, z (row major) holds the
// eigenvectors as columns: z[i * n + k] = component i of the vector of w[k], orthonormal.  Householder reduction to
// tridiagonal form with the transformations accumulated, then the implicit QL iteration with Wilkinson's shift (the
// textbook pair tred2 / tql2, written out here: no LAPACK).  Returns false for n < 1 or if a QL sweep count runs out.
inline bool lz_sym_eig(const double* a, int n, double* w, double* z) {
  if (n < 1 || !a || !w || !z) return false;
  const size_t N = (size_t)n;
  std::vector<double> e(N);
  double* const d = w;
  const auto V = [&](int i, int j) -> double& { return z[(size_t)i * N + (size_t)j]; };
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V(i, j) = 0.5 * (a[(size_t)i * N + j] + a[(size_t)j * N + i]);
  // Householder reduction
  for (int j = 0; j < n; ++j) d[j] = V(n - 1, j);
  for (int i = n - 1; i > 0; --i) {
    double scale = 0.0, h = 0.0;
    for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
    if (scale == 0.0) {
      e[i] = d[i - 1];
      for (int j = 0; j < i; ++j) { d[j] = V(i - 1, j); V(i, j) = 0.0; V(j, i) = 0.0; }
    } else {
      for (int k = 0; k < i; ++k) { d[k] /= scale; h += d[k] * d[k]; }
      double f = d[i - 1], g = std::sqrt(h);
      if (f > 0.0) g = -g;
      e[i] = scale * g;
      h -= f * g;
      d[i - 1] = f - g;
      for (int j = 0; j < i; ++j) e[j] = 0.0;
      for (int j = 0; j < i; ++j) {
        f = d[j];
        V(j, i) = f;
        g = e[j] + V(j, j) * f;
        for (int k = j + 1; k <= i - 1; ++k) { g += V(k, j) * d[k]; e[k] += V(k, j) * f; }
        e[j] = g;
      }
      f = 0.0;
      for (int j = 0; j < i; ++j) { e[j] /= h; f += e[j] * d[j]; }
      const double hh = f / (h + h);
      for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
      for (int j = 0; j < i; ++j) {
        f = d[j];
        g = e[j];
        for (int k = j; k <= i - 1; ++k) V(k, j) -= f * e[k] + g * d[k];
        d[j] = V(i - 1, j);
        V(i, j) = 0.0;
      }
    }
    d[i] = h;
  }
  // accumulate the transformations
  for (int i = 0; i < n - 1; ++i) {
    V(n - 1, i) = V(i, i);
    V(i, i) = 1.0;
    const double h = d[i + 1];
    if (h != 0.0) {
      for (int k = 0; k <= i; ++k) d[k] = V(k, i + 1) / h;
      for (int j = 0; j <= i; ++j) {
        double g = 0.0;
        for (int k = 0; k <= i; ++k) g += V(k, i + 1) * V(k, j);
        for (int k = 0; k <= i; ++k) V(k, j) -= g * d[k];
      }
    }
    for (int k = 0; k <= i; ++k) V(k, i + 1) = 0.0;
  }
  for (int j = 0; j < n; ++j) { d[j] = V(n - 1, j); V(n - 1, j) = 0.0; }
  V(n - 1, n - 1) = 1.0;
  e[0] = 0.0;
  // implicit QL
  for (int i = 1; i < n; ++i) e[i - 1] = e[i];
  e[N - 1] = 0.0;
  double f = 0.0, tst1 = 0.0;
  const double eps = std::numeric_limits<double>::epsilon();
  for (int l = 0; l < n; ++l) {
    tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
    int m = l;
    while (m < n - 1 && std::fabs(e[m]) > eps * tst1) ++m;
    if (m > l) {
      int iter = 0;
      do {
        if (++iter > 200) return false;
        double g = d[l];
        double p = (d[l + 1] - g) / (2.0 * e[l]);
        double r = std::hypot(p, 1.0);
        if (p < 0.0) r = -r;
        d[l] = e[l] / (p + r);
        d[l + 1] = e[l] * (p + r);
        const double dl1 = d[l + 1];
        double h = g - d[l];
        for (int i = l + 2; i < n; ++i) d[i] -= h;
        f += h;
        p = d[m];
        double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
        const double el1 = e[l + 1];
        for (int i = m - 1; i >= l; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          g = c * e[i];
          h = c * p;
          r = std::hypot(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          for (int k = 0; k < n; ++k) {
            h = V(k, i + 1);
            V(k, i + 1) = s * V(k, i) + c * h;
            V(k, i) = c * V(k, i) - s * h;
          }
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
      } while (std::fabs(e[l]) > eps * tst1);
    }
    d[l] += f;
    e[l] = 0.0;
  }
  // ascending order (selection sort: the columns move with their values)
  for (int i = 0; i + 1 < n; ++i) {
    int k = i;
    for (int j = i + 1; j < n; ++j) if (d[j] < d[k]) k = j;
    if (k != i) {
      std::swap(d[i], d[k]);
      for (int j = 0; j < n; ++j) std::swap(V(j, i), V(j, k));
    }
  }
  return true;
}

// Ritz vectors a thick restart of a full active basis of `capacity` vectors keeps.  The residual vector follows them and
// at least one new step must fit behind it: 1 <= r <= capacity - 2.  keep_option > 0 is the caller's count (clamped to
// that range: a stage may have a smaller basis than max_basis), 0 the library's rule - half the basis.  A basis below 3
// cannot restart thick: 0, the caller restarts from the Ritz vector alone (the explicit restart of vqe_lanczos).
inline int lz_keep_count(int capacity, int keep_option) {
  if (capacity < 3) return 0;
  const int r = keep_option > 0 ? keep_option : capacity / 2;
  return std::max(1, std::min(r, capacity - 2));
}

constexpr int kLzMaxEig = 64;              // pairs of one vqe_lanczos_multi call
constexpr int kLzMaxActive = 1024;         // active basis vectors: what one block of k_lz_rotate can stage (vqe_lanczos.h)

// Basis slots of a vqe_lanczos_multi call: locked vectors and the largest active basis, by the budget rule of today.
inline int lz_multi_slots(uint64_t budget_bytes, int n, int max_basis, int n_eig) {
  const int64_t want = (int64_t)std::min(max_basis, kLzMaxActive) + (int64_t)n_eig - 1;
  return lz_basis_capacity(budget_bytes, n, (int)std::min<int64_t>(want, std::numeric_limits<int>::max()));
}

// Active basis vectors of stage e (e vectors locked): min(max_basis, slots - e, 2^n - e), never above kLzMaxActive.
inline int lz_stage_capacity(int slots, int n, int max_basis, int e) {
  const int64_t dim_left = ((int64_t)1 << n) - e;
  const int64_t cap = std::min<int64_t>(std::min<int64_t>(max_basis, kLzMaxActive), std::min<int64_t>((int64_t)slots - e, dim_left));
  return (int)std::max<int64_t>(cap, 0);
}

// The memory rule: the last stage needs 2 active slots (1 where the complement of the locked vectors is one-dimensional);
// the earlier stages then have them too.  false: the call answers VQE_ENOMEM before anything is launched.
inline bool lz_multi_fits(int slots, int n, int max_basis, int n_eig) {
  const int64_t dim_left = ((int64_t)1 << n) - (n_eig - 1);
  return lz_stage_capacity(slots, n, max_basis, n_eig - 1) >= (int)std::min<int64_t>(2, dim_left);
}

// The start vector of stage e is drawn from this seed: stage 0 has the start vector of vqe_lanczos with the same seed.
inline uint64_t lz_stage_seed(uint64_t seed, int e) { return seed ^ ((uint64_t)e * 0xD1B54A32D192ED03ull); }

struct LzMultiOptions {      // vqe_lanczos_multi_opts_t, checked
  int which, n_eig, max_basis, max_matvec, check_every, keep;
  double tol;
  uint64_t seed;
};

enum LzMultiOp { LZM_START = 0, LZM_STEPS = 1, LZM_RESTART = 2, LZM_LOCK = 3, LZM_DONE = 4 };

// What to queue next.  Slots: locked eigenvectors in 0 .. stage-1, active vector j in slot stage + j.
//   START    draw the start vector from `seed`, orthogonalise it (two passes) against slots 0 .. stage-1, normalise it
//            into active slot 0; clear the breakdown flag.
//   STEPS    Lanczos steps j0 .. j1-1.  Step j: w = H v_j - beta_{j-1} v_{j-1} (no second term if j == j0 and no_prev),
//            alpha_j = Re <v_j|w>, w -= alpha_j v_j, two Gram-Schmidt passes against slots 0 .. stage + j, beta_j = |w|,
//            w / beta_j into active slot j + 1 - or, where j + 1 == capacity, in place: the residual vector of a restart.
//            A beta_j below the breakdown threshold stops the run there.  Answer with steps_done().
//   RESTART  active slot q <- sum_i S[i][q] v_i for q < r, i < m (S = s[i * ld + q], real); with_resid: the residual
//            vector becomes active slot r.
//   LOCK     y = sum_i s[i] v_i over the m active vectors, normalised, into slot `stage`; its Rayleigh quotient and true
//            residual by one more application.  Answer with locked().
//   DONE     status(), matvecs(), restarts(), pairs().
struct LzMultiCmd {
  int op, stage, capacity;
  int j0, j1, no_prev;          // STEPS
  int m, r, ld, with_resid;     // RESTART (m, r, ld, with_resid), LOCK (m)
  const double* s;              // RESTART, LOCK: valid until the next call of the machine
  uint64_t seed;                // START
};

class LzMulti {
 public:
  LzMulti(const LzMultiOptions& o, int n, int slots) : o_(o), n_(n), slots_(slots) { begin_stage(0); }

  const LzMultiCmd& cmd() const { return cmd_; }
  int status() const { return budget_ ? 2 : (broke_any_ ? 1 : 0); }
  int matvecs() const { return matvecs_; }
  int restarts() const { return restarts_; }
  int pairs() const { return stage_done_; }
  double theta(int e) const { return theta_[(size_t)e]; }
  double residual(int e) const { return resid_[(size_t)e]; }

  void started() { queue_steps(0, 1); }

  // alpha[j], beta[j] of the steps j0 .. j1-1 of the command (arrays indexed by the step); broke: -1, or the step at
  // which beta was negligible - the steps behind it did not run
  void steps_done(const double* alpha, const double* beta, int broke) {
    const int j0 = cmd_.j0;
    int j1 = cmd_.j1;
    matvecs_ += j1 - j0;
    if (broke >= 0) {
      matvecs_ -= j1 - (broke + 1);
      j1 = broke + 1;
    }
    const size_t ld = (size_t)cap_;
    for (int j = j0; j < j1; ++j) {
      T_[(size_t)j * ld + j] = alpha[j];
      if (j + 1 < cap_) T_[(size_t)j * ld + j + 1] = T_[(size_t)(j + 1) * ld + j] = beta[j];
      ta_[(size_t)j] = alpha[j];
      tb_[(size_t)j] = beta[j];
    }
    k_ = j1;
    beta_last_ = beta[j1 - 1];
    // the wanted Ritz pair of the k x k projected matrix
    int col = 0;
    if (!arrow_) {
      lz_tridiag_extreme(ta_.data(), tb_.data(), k_, o_.which, &ritz_, s_.data());
    } else {
      if (!solve_dense()) return give_up();
      col = o_.which ? k_ - 1 : 0;
      ritz_ = w_[(size_t)col];
      for (int i = 0; i < k_; ++i) s_[(size_t)i] = Z_[(size_t)i * k_ + col];
    }
    if (broke >= 0) {
      broke_any_ = true;
      return queue_lock();
    }
    if (std::fabs(beta_last_ * s_[(size_t)k_ - 1]) <= o_.tol * std::max(1.0, std::fabs(ritz_))) return queue_lock();
    if (matvecs_ >= o_.max_matvec) return give_up();
    if (k_ < cap_) return queue_steps(k_, 0);
    // the active basis is full: restart
    ++restarts_;
    const int r = lz_keep_count(cap_, o_.keep);
    if (!arrow_ && !solve_dense()) return give_up();
    cmd_ = LzMultiCmd{};
    cmd_.op = LZM_RESTART;
    cmd_.stage = e_;
    cmd_.capacity = cap_;
    cmd_.m = k_;
    cmd_.r = std::max(r, 1);
    cmd_.ld = (cmd_.r + 3) & ~3;      // rows padded with zeros to a multiple of 4: the kernel reads four columns at a time
    cmd_.with_resid = r > 0;
    S_.assign((size_t)k_ * cmd_.ld, 0.0);
    for (int q = 0; q < cmd_.r; ++q) {
      const int c = o_.which ? k_ - 1 - q : q;      // the wanted end first
      for (int i = 0; i < k_; ++i) S_[(size_t)i * cmd_.ld + q] = Z_[(size_t)i * k_ + c];
    }
    cmd_.s = S_.data();
  }

  void restarted() {
    const int m = cmd_.m, r = cmd_.with_resid ? cmd_.r : 0;
    std::vector<double> th((size_t)r), b((size_t)r);
    for (int q = 0; q < r; ++q) {
      const int c = o_.which ? m - 1 - q : q;
      th[(size_t)q] = w_[(size_t)c];
      b[(size_t)q] = beta_last_ * Z_[(size_t)(m - 1) * m + c];
    }
    std::fill(T_.begin(), T_.end(), 0.0);
    const size_t ld = (size_t)cap_;
    for (int q = 0; q < r; ++q) {
      T_[(size_t)q * ld + q] = th[(size_t)q];
      T_[(size_t)q * ld + r] = T_[(size_t)r * ld + q] = b[(size_t)q];
    }
    arrow_ = r > 0;
    k_ = r;
    queue_steps(r, 1);
  }

  void locked(double theta, double resid) {
    theta_.push_back(theta);
    resid_.push_back(resid);
    ++stage_done_;
    if (stage_done_ >= o_.n_eig) {
      cmd_ = LzMultiCmd{};
      cmd_.op = LZM_DONE;
      return;
    }
    begin_stage(stage_done_);
  }

 private:
  void begin_stage(int e) {
    e_ = e;
    cap_ = lz_stage_capacity(slots_, n_, o_.max_basis, e);
    T_.assign((size_t)cap_ * cap_, 0.0);
    ta_.assign((size_t)cap_, 0.0);
    tb_.assign((size_t)cap_, 0.0);
    s_.assign((size_t)cap_, 0.0);
    arrow_ = false;
    k_ = 0;
    if (matvecs_ >= o_.max_matvec) return give_up();      // nothing left for this stage
    cmd_ = LzMultiCmd{};
    cmd_.op = LZM_START;
    cmd_.stage = e;
    cmd_.capacity = cap_;
    cmd_.seed = lz_stage_seed(o_.seed, e);
  }
  void queue_steps(int j0, int no_prev) {
    cmd_ = LzMultiCmd{};
    cmd_.op = LZM_STEPS;
    cmd_.stage = e_;
    cmd_.capacity = cap_;
    cmd_.j0 = j0;
    cmd_.j1 = std::min(std::min(j0 + o_.check_every, cap_), j0 + (o_.max_matvec - matvecs_));
    cmd_.no_prev = no_prev;
  }
  void queue_lock() {
    cmd_ = LzMultiCmd{};
    cmd_.op = LZM_LOCK;
    cmd_.stage = e_;
    cmd_.capacity = cap_;
    cmd_.m = k_;
    cmd_.s = s_.data();
  }
  bool solve_dense() {
    A_.resize((size_t)k_ * k_);
    w_.resize((size_t)k_);
    Z_.resize((size_t)k_ * k_);
    for (int i = 0; i < k_; ++i)
      for (int j = 0; j < k_; ++j) A_[(size_t)i * k_ + j] = T_[(size_t)i * cap_ + j];
    return lz_sym_eig(A_.data(), k_, w_.data(), Z_.data());
  }
  // status 2 with the pairs locked so far: the budget is spent (or lz_sym_eig ran out of sweeps - not observed)
  void give_up() {
    budget_ = true;
    cmd_ = LzMultiCmd{};
    cmd_.op = LZM_DONE;
  }

  LzMultiOptions o_;
  int n_, slots_;
  int e_ = 0, cap_ = 0, k_ = 0, stage_done_ = 0, matvecs_ = 0, restarts_ = 0;
  bool arrow_ = false, broke_any_ = false, budget_ = false;
  double beta_last_ = 0.0, ritz_ = 0.0;
  LzMultiCmd cmd_{};
  std::vector<double> T_, ta_, tb_, s_, A_, w_, Z_, S_, theta_, resid_;
};

}  // namespace vqe
