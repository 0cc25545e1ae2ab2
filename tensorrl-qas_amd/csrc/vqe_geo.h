// vqe_geo.h - the constants that the kernels (vqe_device.h, vqe_reg.h) and the host-side planners (ham_layout.h,
// dm_host.h) share: workgroup geometry, gate records, and the parameters of the Hamiltonian layout.  Plain C++: it
// compiles with a host compiler alone as well as with hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VQE_HD __host__ __device__
#else
#define VQE_HD
#endif

namespace vqe {

constexpr int kThreads = 256;   // default workgroup size (n <= 11 and the streaming path)

// Workgroup geometry of the LDS-resident kernels.
//  * n <= 11: 256 threads, registers capped for 4 waves per SIMD (4 workgroups per CU fit the
//    LDS): measured at n = 11 +31 % over 2 waves per SIMD although the cap costs spills - the
//    vector-memory, LDS and VALU pipes of the energy step overlap better across more waves;
//  * n = 12: 256 threads x 16 amplitudes, 2 workgroups per CU (LDS bound), 256 VGPRs.  The
//    512-thread variant (8 amplitudes per thread, 4 waves per SIMD in 128 VGPRs) was measured
//    15 % slower: 124 spilled registers and one more re-layout per ~3 rotations;
//  * n = 13: 512 threads x 16 amplitudes, one workgroup per CU.
#ifndef VQE_WIDE_MIN
#define VQE_WIDE_MIN 13
#endif
constexpr int kWideMinQubits = VQE_WIDE_MIN;   // 512-thread workgroups from this size on

#ifndef VQE_ONE_WAVE_MAX
#define VQE_ONE_WAVE_MAX 9
#endif
// Up to this size an environment is ONE wavefront (64 threads, 4 amplitudes per thread at 8 qubits).  With four waves
// per environment three of them sit at a barrier while wave 0 runs the optimiser update, and at this size that update
// is most of an evaluation: one-wave workgroups keep 16 environments per CU busy instead of 4 (8 qubits, 20 gates:
// 46.9 -> 92.4 M evaluations/s; 150 gates: 12.9 -> 13.2 M; 129 variables: 6.3 -> 5.8 M at 4096 environments, 6.4 M
// at 16384 - the price of having no second wave for the workgroup-wide update).
constexpr int kOneWaveMaxQubits = VQE_ONE_WAVE_MAX;

#ifndef VQE_ONE_WAVE_REG
#define VQE_ONE_WAVE_REG 0      // 1: 10 qubits on the register path with one wave (16 amplitudes per thread) - parity green, 0..9 % slower than four waves x 4 amplitudes
#endif
VQE_HD constexpr bool geo_one_wave(int n) { return n <= kOneWaveMaxQubits || (VQE_ONE_WAVE_REG && n == 10); }
VQE_HD constexpr int geo_lt(int n) { return n >= kWideMinQubits ? 9 : (geo_one_wave(n) ? 6 : 8); }

#ifndef VQE_WPS_SMALL
#define VQE_WPS_SMALL 2     // n <= 9 (one wave per environment): all 256 registers - at 128 these kernels spilled 470..690 B per lane; eight environments per CU without spills beat sixteen with them by 18..32 %
#endif
#ifndef VQE_WPS10
#define VQE_WPS10 4
#endif
#ifndef VQE_WPS11
#define VQE_WPS11 3     // n = 11: 170 registers per wave instead of 128 (464 B of spills), three workgroups per CU (the LDS rarely admits a fourth): +2..3 %
#endif
template <int N>
struct Geo {
  static constexpr int NT = 1 << geo_lt(N);        // threads per workgroup
  static constexpr int LT = geo_lt(N);             // log2(NT)
  static constexpr int NW = NT / 64;               // waves per workgroup
  static constexpr int WPS = N == 11 ? VQE_WPS11 : (N == 10 ? (VQE_ONE_WAVE_REG ? 2 : VQE_WPS10) : (N <= 9 ? VQE_WPS_SMALL : 2));      // waves per SIMD asked of the register allocator
};

constexpr int kRegMinQubits = 10;   // register path (vqe_reg.h) from this size on

enum : int { G_CNOT = 0, G_RX = 1, G_RY = 2, G_RZ = 3, G_DEPOL1 = 4, G_DEPOL2 = 5, G_RXX = 6, G_RYY = 7, G_RZZ = 8 };
// two-qubit Pauli rotations exp(+i theta/2 P_q0 P_q1) (fields q0, q1, pidx) / any gate that carries a parameter
VQE_HD constexpr bool gate_is_rot2(int k) { return k >= G_RXX && k <= G_RZZ; }
VQE_HD constexpr bool gate_is_rot(int k) { return (k >= G_RX && k <= G_RZ) || gate_is_rot2(k); }
struct GateRec { int32_t kind, q0, q1, pidx; };           // as uploaded by the host

// The circuit COBYLA sees in an environment step (CircuitEnv.step of the reference,
// environments/environment_qulacs_TN_notin_agent.py:283-291,452-482): circuit g[0..G) WITHOUT the gate the action just
// added, g[new_gate].  Gates [skip, skip_end) are left out; hole = parameter index of the new gate if it is a rotation
// (its angle is not a variable), else -1.  The noise channel construct_ansatz puts behind every gate belongs to that
// gate, so the pre-action circuit contains neither (VQE_qulacs_TN_notin_RL_noise.py:26-28,40-50): a DEPOL1 behind a
// one-qubit rotation on the same qubit, a DEPOL2 behind a CNOT on the same (q0, q1).  RXX / RYY / RZZ on purpose not:
// the reference's SU(4) ansatz builder attaches no channel to its gates (VQE_qulacs_su4.py:13-63), so a DEPOL2 behind
// a new two-qubit rotation is a gate of its own and stays in.  No new gate: the empty range [-1, 0).
struct PreAction { int skip, skip_end, hole; };
VQE_HD inline PreAction pre_action(const GateRec* g, int G, int new_gate) {
  if (new_gate < 0) return PreAction{-1, 0, -1};
  const GateRec r = g[new_gate];
  PreAction pa{new_gate, new_gate + 1, gate_is_rot(r.kind) ? r.pidx : -1};
  if (new_gate + 1 < G) {
    const GateRec fo = g[new_gate + 1];
    if ((fo.kind == G_DEPOL1 && r.kind >= G_RX && r.kind <= G_RZ && fo.q0 == r.q0) ||
        (fo.kind == G_DEPOL2 && r.kind == G_CNOT && fo.q0 == r.q0 && fo.q1 == r.q1))
      pa.skip_end = new_gate + 2;
  }
  return pa;
}

// Depth of the energy step's table ring, and so the multiple to which the host pads the real-table sections of the
// group list (by size: the shallower ring frees 32 registers where the kernel sits at its register cap -
// n = 11 ... 13: +1..2 % - and costs 2..3 % where it does not)
VQE_HD constexpr int energy_pd(int n) { return n >= 11 ? 2 : 4; }

// LDS slot of canonical index p under the bank swizzle `swz` (HamDev::swz / HamLayout::swz)
VQE_HD inline uint32_t swz_slot(uint64_t swz, uint32_t p) {
  return p ^ (uint32_t)((swz >> (((p >> 4) & 15u) << 2)) & 15u);
}
constexpr int kUnitMinQubits = 8;             // below: a group has no more pairs than a workgroup has threads
constexpr int kUnitTrip = 4;                  // units per trip of the unit loop
constexpr int kUnitUnroll = 3 * kUnitTrip;    // HamDev::n_units is padded to a multiple of this (three trips per turn of the loop)
// The loop prefetches two trips beyond the one it accumulates: the arrays it reads (ham_layout.h: unit_arrays) end
// with this many zero units, so that the last turns prefetch without clamping their offsets
constexpr int kUnitAhead = 2 * kUnitTrip;
// Sign-sum entries below kUnitZeroTol x sum_k |c_k| are rounding residues of sums that cancel exactly in real
// arithmetic (3w - w - w - w is not 0 in floating point) and count as zero.
constexpr double kUnitZeroTol = 0x1p-44;       // 5.7e-14 relative: far above the residues (~1e-16), far below any term

}  // namespace vqe
