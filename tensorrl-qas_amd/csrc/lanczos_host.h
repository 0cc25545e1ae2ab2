// lanczos_host.h - host logic of the device Lanczos solver (vqe_lanczos, csrc/vqe_lanczos.h).
// Host only, no HIP: tests/cpp/lanczos_host_check.cpp compiles it with g++ and holds it without a GPU.
//   lz_tridiag_extreme  the lowest or highest eigenpair of the symmetric tridiagonal T the recurrence builds
//                       (bisection on the Sturm count, then inverse iteration; no LAPACK);
//   lz_decide           the stop rule, a pure function of (alpha, beta, options, counters);
//   lz_basis_capacity   how many basis vectors the solver keeps.
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

}  // namespace vqe
