// mps2qc_plan.h - what the host decides before an MPS -> PQC fit is launched: argument checks, the runs of mutually
// disjoint gates, threads per fit, the LDS layout that k_fit trusts, the learning-rate schedule.  Host only - integer
// and double arithmetic on std::vector, no HIP - so that the planner / kernel contract written down on FitLds is
// checked without a GPU (tests/cpp/mps2qc_plan_check.cpp).  mps2qc_fit.hip uploads and launches what this file plans.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace mps2qc {

constexpr int kMat = 16;          // complex entries of a gate
constexpr int kSlotMats = 10;     // LDS matrices per 16-lane update group
constexpr int kLdsLimit = 160 * 1024;

// Both entry points: bounds, null checks, and lo[k] = n - 2 - sites[k], the low bit of gate k's qubit pair
// (site 0 is the most significant bit).  false: `err` holds the message.
inline bool check_fit_args(const char* fn, int n, int n_max, int G, int batch, int max_iter, const int32_t* sites,
                           const void* target, const void* init_gates, std::vector<int>& lo, std::string& err) {
  char msg[256];
  if (n < 2 || n > n_max || G < 1 || batch < 1 || max_iter < 1 || !sites || !target || !init_gates) {
    snprintf(msg, sizeof msg, "%s: bad argument (2 <= n <= %d, G, batch, max_iter >= 1)", fn, n_max);
    err = msg;
    return false;
  }
  lo.resize(G);
  for (int k = 0; k < G; ++k) {
    if (sites[k] < 0 || sites[k] > n - 2) {
      snprintf(msg, sizeof msg, "%s: gate %d on sites (%d,%d) outside the register", fn, k, sites[k], sites[k] + 1);
      err = msg;
      return false;
    }
    lo[k] = n - 2 - sites[k];
  }
  return true;
}

// [first, count] of every maximal run of mutually disjoint gates (a brickwork half layer), in gate order: a run ends
// where the next gate shares a qubit with one of its gates.
inline std::vector<int> disjoint_runs(const std::vector<int>& lo) {
  std::vector<int> runs;
  unsigned used = 0;
  for (int k = 0; k < (int)lo.size(); ++k) {
    const unsigned bits = 3u << lo[k];
    if (runs.empty() || (used & bits)) {
      runs.push_back(k), runs.push_back(0);
      used = 0;
    }
    used |= bits;
    ++runs.back();
  }
  return runs;
}

// threads per fit: enough waves per SIMD to hide the LDS latency of the gate sweeps
constexpr int threads_per_fit(int n) { return n <= 8 ? 64 : n <= 10 ? 256 : 512; }

// Bias-corrected learning rate of step it + 1 (stiefel_opt.py:333-335); t = 1 when frozen.
inline double lr_schedule(double lr, double beta1, double beta2, bool frozen, int it) {
  const double t = frozen ? 1.0 : (double)(it + 1);
  return lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t));
}

// Dynamic LDS of k_fit<N, NT>, bytes from its start.  The kernel trusts these offsets completely; the contract:
//   [0, 2 * 2^n * 16)   psi, phi        double2
//   off_u, off_e        [G][16] each    double2  gates, environments
//   off_red             [red_slots][NT/64 * 64]  double   MFMA partials; red_slots >= 2 (double buffering), one per gate
//                                       of the largest run when the half-layer scheme runs and LDS has room
//   off_sc              [2 * 16]        double   one complex partial per wave (<= 16 waves)
//   off_dn              [G, even]       double   norm of every gate's change
//   off_lo              [G, to 4]       int      lo[k]
//   off_grp             [runs, to 4]    int      disjoint_runs
//   off_scratch         [min(NT/16, 16)][kSlotMats][16] double2  update operands: 0 = overlaid on psi / phi (idle during
//                                       the update) exactly when the two states are at least that large
// All regions are disjoint (but for that overlay), 16-byte aligned and end at `total` <= kLdsLimit.
struct FitLds {
  int off_u, off_e, off_red, off_sc, off_dn, off_lo, off_grp, off_scratch;
  int red_slots;
  size_t total;
};

inline size_t fit_scratch_bytes(int NT) { return (size_t)(NT / 16 < 16 ? NT / 16 : 16) * kSlotMats * kMat * 16; }

// false: the layout does not fit (`err` holds the message).  runs: disjoint_runs(lo); grouped: the half-layer scheme
// will run; red2: keep two partial buffers even where LDS has room for more.
inline bool plan_fit_lds(int n, int G, const std::vector<int>& runs, int NT, bool grouped, bool red2, FitLds& L,
                         std::string& err) {
  const size_t states = 2 * ((size_t)1 << n) * 16, gates = (size_t)G * kMat * 16, red = (size_t)(NT / 64) * 64 * 8;
  const size_t sc = 2 * 16 * 8, dn = (size_t)((G + 1) & ~1) * 8, lo = (size_t)((G + 3) & ~3) * 4;
  const size_t grp = ((runs.size() + 3) & ~(size_t)3) * 4;
  const size_t scratch = states >= fit_scratch_bytes(NT) ? 0 : fit_scratch_bytes(NT);      // 0: overlaid
  const size_t rest = states + 2 * gates + sc + dn + lo + grp + scratch;
  int big = 2;
  for (size_t g = 1; g < runs.size(); g += 2) big = runs[g] > big ? runs[g] : big;
  L.red_slots = grouped && !red2 && rest + big * red <= (size_t)kLdsLimit ? big : 2;

  size_t off = states;
  L.off_u = (int)off, off += gates;
  L.off_e = (int)off, off += gates;
  L.off_red = (int)off, off += L.red_slots * red;
  L.off_sc = (int)off, off += sc;
  L.off_dn = (int)off, off += dn;
  L.off_lo = (int)off, off += lo;
  L.off_grp = (int)off, off += grp;
  L.off_scratch = scratch ? (int)off : 0, off += scratch;
  L.total = off;
  if (off > (size_t)kLdsLimit) {
    char msg[256];
    snprintf(msg, sizeof msg, "mps2qc_fit_brickwork: %d gates at %d qubits need %zu B of LDS (limit %d)", G, n, off,
             kLdsLimit);
    err = msg;
    return false;
  }
  return true;
}

}  // namespace mps2qc
