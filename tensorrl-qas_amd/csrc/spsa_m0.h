// spsa_m0.h - Adam-SPSA: the schedule scalars of one iteration and the update of one element.
//
// Host and device: k_lds_minimize_spsa (vqe_spsa.h) calls these functions, and so does tests/cpp/spsa_host_check.cpp,
// built with plain g++.  tests/spsa_helpers.py restates the algorithm statement for statement:
//
//   x = x0;  m = v = 0;  b1p = b2p = 1
//   for k = 0 .. K-1:
//       a_k = a / (k + 1 + stability)^alpha
//       c_k = c / (k + 1)^gamma
//       key = noise_key(seed, b, k)                       (b: position in the batch)
//       D_j = +1 if noise_uniform_k(key, j) < 0.5 else -1   (j = 0 .. P-1; D_hole = 0)
//       f+ = E(x + c_k D)   evaluation id eval_base + 2k
//       f- = E(x - c_k D)   evaluation id eval_base + 2k + 1
//       g_j = (f+ - f-) / (2 c_k) * D_j
//       b1k = beta_1 / (k + 1)^lamda
//       m = b1k m + (1 - b1k) g
//       v = beta_2 v + (1 - beta_2) g*g
//       b1p *= b1k;  b2p *= beta_2
//       x_j -= a_k * (m_j / (1 - b1p)) / (sqrt(v_j / (1 - b2p)) + eps)
//
// Everything that does not depend on j - the three pow calls, the products, the bias corrections, the gradient scale -
// is formed once per iteration (spsa_begin_iteration, spsa_close_iteration), identically on every thread; the element
// update (spsa_update_element) is a dozen operations without a transcendental besides one sqrt.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SPSA_HD __host__ __device__
#else
#define SPSA_HD
#endif

// No contraction into fused multiply-adds in this header (as cobyla_m0.h): the device then rounds every operation as the
// host build and the numpy restatement do, and what is left between them is the last place of pow and sqrt.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vqe {

// (the fields of vqe_spsa_opts_t, include/vqe_hip.h, in its order)
struct SpsaOpts {
  int32_t maxiter;
  double a, alpha, stability, c, gamma, beta_1, beta_2, lamda, eps;
  uint64_t seed;
};

SPSA_HD inline SpsaOpts spsa_default_opts() { return SpsaOpts{100, 0.1, 0.602, 0.0, 0.1, 0.101, 0.9, 0.999, 0.0, 1e-8, 0}; }

// Why these options are refused, or nullptr
SPSA_HD inline const char* spsa_bad_option(const SpsaOpts& o) {
  const double all[9] = {o.a, o.alpha, o.stability, o.c, o.gamma, o.beta_1, o.beta_2, o.lamda, o.eps};
  for (int i = 0; i < 9; ++i)
    if (!(all[i] - all[i] == 0.0)) return "Adam-SPSA options must be finite";      // (inf - inf and NaN - NaN are NaN)
  if (o.maxiter < 0) return "Adam-SPSA needs maxiter >= 0";
  if (!(o.a > 0.0)) return "Adam-SPSA needs a > 0";
  if (!(o.c > 0.0)) return "Adam-SPSA needs c > 0";
  if (!(o.eps > 0.0)) return "Adam-SPSA needs eps > 0";
  if (o.alpha < 0.0) return "Adam-SPSA needs alpha >= 0";
  if (o.gamma < 0.0) return "Adam-SPSA needs gamma >= 0";
  if (o.lamda < 0.0) return "Adam-SPSA needs lamda >= 0";
  if (o.stability < 0.0) return "Adam-SPSA needs stability >= 0";
  if (!(o.beta_1 >= 0.0 && o.beta_1 < 1.0)) return "Adam-SPSA needs beta_1 in [0, 1)";
  if (!(o.beta_2 >= 0.0 && o.beta_2 < 1.0)) return "Adam-SPSA needs beta_2 in [0, 1)";
  return nullptr;
}

// What the optimiser carries from one iteration to the next besides its vectors, and the scalars of the running one
struct SpsaIter {
  double b1p, b2p;            // products of b1k and of beta_2 over the iterations made
  double a_k, c_k, b1k;       // of iteration k (spsa_begin_iteration)
  double gs, mden, vden;      // (f+ - f-) / (2 c_k), 1 - b1p, 1 - b2p (spsa_close_iteration)
};
SPSA_HD inline SpsaIter spsa_start() { return SpsaIter{1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0}; }

SPSA_HD inline void spsa_begin_iteration(SpsaIter& s, const SpsaOpts& o, int k) {
  const double k1 = (double)(k + 1);
  s.a_k = o.a / pow(k1 + o.stability, o.alpha);
  s.c_k = o.c / pow(k1, o.gamma);
  s.b1k = o.beta_1 / pow(k1, o.lamda);
}

// both energies of the iteration are known
SPSA_HD inline void spsa_close_iteration(SpsaIter& s, const SpsaOpts& o, double fp, double fm) {
  s.gs = (fp - fm) / (2.0 * s.c_k);
  s.b1p *= s.b1k;
  s.b2p *= o.beta_2;
  s.mden = 1.0 - s.b1p;
  s.vden = 1.0 - s.b2p;
}

// Element j: D is its perturbation sign (+1, -1, or 0 for a parameter that is not optimised, which then never moves)
SPSA_HD inline void spsa_update_element(const SpsaIter& s, const SpsaOpts& o, double D, double& x, double& m, double& v) {
  const double g = s.gs * D;
  m = s.b1k * m + (1.0 - s.b1k) * g;
  v = o.beta_2 * v + (1.0 - o.beta_2) * g * g;
  x -= s.a_k * (m / s.mden) / (sqrt(v / s.vden) + o.eps);
}

}  // namespace vqe

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
