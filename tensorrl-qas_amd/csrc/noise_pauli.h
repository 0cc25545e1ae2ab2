// noise_pauli.h - a Pauli channel in a noise slot of the mode 0 sampler (vqe_set_noise_pauli).
//
// The depolarising draw splits the slot's probability evenly over the 3 or 15 non-identity Paulis; a table gives every
// Pauli a probability of its own: rho -> w_0 rho + sum_k w_k P_k rho P_k, w_0 the remainder.  Code k: 1 = X, 2 = Y,
// 3 = Z at a G_DEPOL1 gate; k = a | b << 2 at a G_DEPOL2 gate, a on q0 and b on q1 (the code patch_noise_wave and
// k_s_compile consume).  The draw:
//   cum_0 = 0, cum_k = cum_{k-1} + w_k, in this order in double;
//   code(u) = 0 where u >= cum_m, else the smallest k with u < cum_k (an entry with w_k = 0 is never selected).
// Plain C++: the kernels (vqe_device.h, vqe_stream.h), the host (vqe_api.hip) and tests/cpp/noise_pauli_check.cpp
// include this one file.
#pragma once
#include <stdint.h>

#ifndef VQE_HD
#if defined(__HIPCC__)
#define VQE_HD __host__ __device__
#else
#define VQE_HD
#endif
#endif

namespace vqe {

// The thresholds of both slots as the kernels read them (a device buffer of the handle; NoiseCfg holds its address).
// has1 / has2 = 0: that slot has no table and draws by the depolarising rule of p1 / p2.
struct NoisePauliTab {
  double cum1[3];
  double cum2[15];
  int32_t has1, has2;
};

// cum[k - 1] = w_1 + ... + w_k, accumulated in k order; the return value is the total cum_m (0 for m = 0)
VQE_HD inline double pauli_cumulate(const double* w, int m, double* cum) {
  double c = 0.0;
  for (int k = 0; k < m; ++k) { c += w[k]; cum[k] = c; }
  return c;
}

// The code of the draw u.  cum is non-decreasing, so the thresholds at or below u are the leading ones: their count is
// the code minus one, and a count of m is the identity.  Branch-free; P: any pointer to double (the kernels pass the
// constant address space, so the loads are scalar).
template <class P>
VQE_HD inline int pauli_code(double u, P cum, int m) {
  int below = 0;
  for (int k = 0; k < m; ++k) below += u >= cum[k] ? 1 : 0;
  return below == m ? 0 : 1 + below;
}

// What vqe_set_noise_pauli accepts: every entry a number in [0, 1] and a total of at most 1 + 1e-12
VQE_HD inline bool pauli_weights_ok(const double* w, int m) {
  double c = 0.0;
  for (int k = 0; k < m; ++k) {
    if (!(w[k] >= 0.0 && w[k] <= 1.0)) return false;      // (a NaN fails both comparisons)
    c += w[k];
  }
  return c <= 1.0 + 1e-12;
}

}  // namespace vqe
