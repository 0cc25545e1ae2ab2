// noise_grad_host.h - host rules of the gradients of frozen Pauli-noise realisations (vqe_set_noise_grad):
// whether a gradient / L-BFGS call is served, and how far the evaluation counter moves after a run.  Plain C++, no
// device code: vqe_api.hip applies it, tests/cpp/noise_grad_check.cpp checks it without a GPU.
#pragma once
#include <cstdint>

namespace vqe {

constexpr int kNoiseGradMaxReal = 4096;

// What the refusal test of the adjoint entry points sees of a handle (after the Kraus test, before the tests for the
// exact channel mode, shot noise and shards, which stay what they were).
struct NoiseGradState {
  int n_real;        // T of vqe_set_noise_grad (0: off)
  int noise_mode;    // 0 Pauli trajectories, 1 exact channel
  bool pauli_on;     // p1 / p2 or a table's total is positive
  bool lds_path;     // n <= 13
};
enum NoiseGradVerdict : int {
  NG_NOISELESS = 0,      // no Pauli noise: the noiseless kernels, whatever the switch says
  NG_SERVED = 1,         // the mean over T frozen realisations
  NG_REFUSED_OFF = 2,    // Pauli noise and the switch off (or mode 1): refused as before the switch existed
  NG_REFUSED_PATH = 3,   // switch on, n >= 14
};
inline NoiseGradVerdict noise_grad_verdict(const NoiseGradState& s) {
  if (!s.pauli_on) return NG_NOISELESS;
  if (s.n_real <= 0 || s.noise_mode != 0) return NG_REFUSED_OFF;
  if (!s.lds_path) return NG_REFUSED_PATH;
  return NG_SERVED;
}

// Evaluation ids a SERVED run consumes - what eval_base grows by afterwards.  A gradient run reads ids
// eval_base .. eval_base + T - 1 and moves on unless the counter is held; an L-BFGS run reads the same T ids at every
// evaluation and always moves on; an environment step reads one more id (eval_base + T) for its closing energy.
enum class NoiseGradRun { Gradient, Lbfgs, EnvStepLbfgs };
inline uint64_t noise_grad_consumed(NoiseGradRun run, int n_real, bool hold) {
  switch (run) {
    case NoiseGradRun::Gradient: return hold ? 0u : (uint64_t)n_real;
    case NoiseGradRun::Lbfgs: return (uint64_t)n_real;
    case NoiseGradRun::EnvStepLbfgs: return (uint64_t)n_real + 1u;
  }
  return 0u;
}

}  // namespace vqe
