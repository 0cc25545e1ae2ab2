// env_step_host.h - the host halves of an environment step, shared by the drivers that run the optimiser from the host
// (stream_run and dm_run, vqe_api.hip): build the pre-action circuit COBYLA sees, and put its optimum back into the
// full circuit's parameter layout.  The rule itself is pre_action (vqe_geo.h).  The fused kernel does NOT call it:
// k_lds_minimize (vqe_device.h) holds a hand-kept copy of the rule in its prologue, and a change must land in both.
// Plain C++, no HIP: checked on the CPU by tests/cpp/env_step_check.cpp.
#pragma once
#include "vqe_geo.h"

#include <vector>

namespace vqe {

// Appends the pre-action circuit of g[0..G) (parameters theta[0..P)) to gates2 / x0: the gates outside
// [skip, skip_end), every rotation's pidx above the hole one lower, theta without the hole's entry.
inline PreAction pre_action_circuit(const GateRec* g, int G, int new_gate, const double* theta, int P,
                                    std::vector<GateRec>& gates2, std::vector<double>& x0) {
  const PreAction pa = pre_action(g, G, new_gate);
  for (int i = 0; i < G; ++i) {
    if (i >= pa.skip && i < pa.skip_end) continue;
    GateRec r = g[i];
    if (gate_is_rot(r.kind) && pa.hole >= 0 && r.pidx > pa.hole) r.pidx -= 1;
    gates2.push_back(r);
  }
  for (int j = 0; j < P; ++j)
    if (j != pa.hole) x0.push_back(theta[j]);
  return pa;
}

// The inverse after the optimiser: xopt holds the pre-action circuit's parameters.  xraw[0..P): the hole's entry from
// theta, the others from xopt; x: the same, rounded to float32 in an environment step (the state tensor's dtype).
inline void merge_optimum(const double* theta, int P, int hole, const double* xopt, bool env_step, double* x, double* xraw) {
  for (int j = 0, k = 0; j < P; ++j) {
    const double v = j == hole ? theta[j] : xopt[k++];
    xraw[j] = v;
    x[j] = env_step ? (double)(float)v : v;
  }
}

}  // namespace vqe
