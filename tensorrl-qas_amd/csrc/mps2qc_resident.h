// mps2qc_resident.h - what the host decides before a resident streaming fit (mps2qc_fit_brickwork_resident) is
// launched: the option check, the buffer sizes and the number of step sequences the host loop may enqueue, plus the one
// index function the host shares with a kernel (sfd_bitrev).  Integer arithmetic only, no HIP, so that all of it is
// checked without a GPU (tests/cpp/stream_fit_host_check.cpp).  mps2qc_resident_kernels.h launches what this file plans.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/mps2qc_hip.h"

#if defined(__HIPCC__)
#define SFD_HD __host__ __device__
#else
#define SFD_HD
#endif

namespace mps2qc {

constexpr int kSfdThreads = 256;      // block size of every k_sfd_* kernel (the k_sf_* sweeps use the same)

// i with its n low bits reversed: the index, in the engine's order (qubit 0 = bit 0), of the amplitude that quimb's
// order (site 0 = most significant bit) holds at i - and the other way round, the map is an involution.
SFD_HD inline size_t sfd_bitrev(size_t i, int n) {
  size_t r = 0;
  for (int b = 0; b < n; ++b) r |= ((i >> b) & (size_t)1) << (n - 1 - b);
  return r;
}

inline mps2qc_resident_opts_t sfd_default_opts() { return mps2qc_resident_opts_t{0, 0, 8, -1}; }

// false: `err` holds the message.  (That a target_on_device pointer is device memory is checked where HIP is.)
inline bool sfd_check_opts(const mps2qc_resident_opts_t& o, std::string& err) {
  char msg[256];
  const char* what = nullptr;
  if (o.target_on_device != 0 && o.target_on_device != 1) what = "target_on_device must be 0 or 1";
  else if (o.target_little_endian != 0 && o.target_little_endian != 1) what = "target_little_endian must be 0 or 1";
  else if (o.check_every < 1) what = "check_every must be >= 1";
  else if (o.use_graph < -1 || o.use_graph > 1) what = "use_graph must be -1, 0 or 1";
  if (!what) return true;
  snprintf(msg, sizeof msg, "mps2qc_fit_brickwork_resident: %s (got %d, %d, %d, %d)", what, o.target_on_device,
           o.target_little_endian, o.check_every, o.use_graph);
  err = msg;
  return false;
}

// Element counts (not bytes) of the per-fit device state.  A sweep over amplitudes has sfd_blocks_amp blocks, one over
// 4-vectors sfd_blocks_vec; the backward sweep of gate k of fit b leaves 16 complex partials per block at
// [b][k][block][16], the overlap one per block at [b][block].
inline size_t sfd_blocks(size_t items) { return (items + kSfdThreads - 1) / kSfdThreads; }
inline size_t sfd_blocks_amp(int n) { return sfd_blocks((size_t)1 << n); }
inline size_t sfd_blocks_vec(int n) { return sfd_blocks(((size_t)1 << n) / 4); }
inline size_t sfd_state_count(int n, int batch) { return (size_t)batch << n; }
inline size_t sfd_env_partial_count(int n, int G, int batch) { return (size_t)batch * (size_t)G * sfd_blocks_vec(n) * 16; }
inline size_t sfd_ov_partial_count(int n, int batch) { return (size_t)batch * sfd_blocks_amp(n); }

// The most step sequences the host loop puts on the stream: it enqueues check_every at a time and reads the stop
// flags after each round; the update kernel has stopped every fit once max_iter steps ran.
inline long long sfd_max_steps_enqueued(int max_iter, int check_every) {
  return ((long long)max_iter + check_every - 1) / check_every * check_every;
}

}  // namespace mps2qc
