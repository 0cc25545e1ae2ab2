// noise_grad_host.h - host rules of the gradients of frozen Pauli-noise realisations (vqe_set_noise_grad):
// whether a gradient / L-BFGS call is served, and how far the evaluation counter moves after a run.  Plain C++, no
// device code: vqe_api.hip applies it, tests/cpp/noise_grad_check.cpp checks it without a GPU.  Since DESIGN 4.21 also the
// verdict and the chunk planner of the streaming form (vqe_set_stream_noise_grad; tests/cpp/stream_noise_grad_check.cpp).
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
  bool stream_on = false;   // n >= 14 and vqe_set_stream_noise_grad switched the streaming form on
};
enum NoiseGradVerdict : int {
  NG_NOISELESS = 0,      // no Pauli noise: the noiseless kernels, whatever the switch says
  NG_SERVED = 1,         // the mean over T frozen realisations
  NG_REFUSED_OFF = 2,    // Pauli noise and the switch off (or mode 1): refused as before the switch existed
  NG_REFUSED_PATH = 3,   // switch on, n >= 14, the streaming form off
  NG_SERVED_STREAM = 4,  // switch on, n >= 14, the streaming form on: the same mean, as virtual streams in HBM
};
inline NoiseGradVerdict noise_grad_verdict(const NoiseGradState& s) {
  if (!s.pauli_on) return NG_NOISELESS;
  if (s.n_real <= 0 || s.noise_mode != 0) return NG_REFUSED_OFF;
  if (!s.lds_path) return s.stream_on ? NG_SERVED_STREAM : NG_REFUSED_PATH;
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

// ---- the (circuit, realisation) grid of the streaming form (vqe_set_stream_noise_grad) ----
// The B * T pairs are numbered v = b * T + t (virtual streams) and run `resident` at a time: chunk c holds the pairs
// [c * resident, min((c + 1) * resident, B * T)), in that order.  A chunk is the y extent of a grid: at most 65535.
constexpr int kNoiseGradMaxChunk = 65535;
struct NoiseGradPair { int b, t; };
struct NoiseGradChunks {
  int64_t pairs;     // B * T
  int resident;      // pairs of a full chunk: min(max(cap, 1), pairs, 65535), at least 1
  int chunks;        // ceil(pairs / resident); 0 for an empty batch
};
inline NoiseGradChunks noise_grad_chunks(int B, int T, int64_t cap) {
  const int64_t pairs = (B > 0 && T > 0) ? (int64_t)B * (int64_t)T : 0;
  int64_t r = cap < 1 ? 1 : cap;
  if (r > pairs) r = pairs;
  if (r > kNoiseGradMaxChunk) r = kNoiseGradMaxChunk;
  if (r < 1) r = 1;
  return NoiseGradChunks{pairs, (int)r, (int)((pairs + r - 1) / r)};
}
// the pairs [lo, hi) of chunk c (lo == hi for a chunk that does not exist)
inline void noise_grad_chunk_range(const NoiseGradChunks& p, int c, int64_t* lo, int64_t* hi) {
  int64_t a = (c < 0 ? 0 : (int64_t)c) * p.resident, e = a + p.resident;
  if (a > p.pairs) a = p.pairs;
  if (e > p.pairs) e = p.pairs;
  *lo = a;
  *hi = e;
}
inline NoiseGradPair noise_grad_pair(int64_t v, int T) { return NoiseGradPair{(int)(v / T), (int)(v % T)}; }

}  // namespace vqe
