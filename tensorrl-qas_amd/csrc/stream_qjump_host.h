// stream_qjump_host.h - the round structure of quantum-jump trajectories on the streaming path (vqe_stream_qjump.h),
// for the host and the device alike; checked without a GPU by tests/cpp/sq_host_check.cpp.
//
// A compiled trajectory (qj_compile, vqe_qjump.h) is a list of records: rotations, QJ_JUMP1, QJ_JUMP2 + QJ_TAIL.  The
// streaming path runs all resident (circuit, trajectory) states in lock-step rounds r = 0 .. R: round r applies the
// r-th run of rotation records of every state, then its r-th jump.  A circuit with J jumps has J + 1 runs (any of them
// may be empty); in the rounds beyond J it idles.  The rounds partition the record list in order:
//   run r = [lo_r, hi_r),  the jump of round r at hi_r (r < J; one record, or two with its QJ_TAIL),  lo_{r+1} behind it,
//   lo_0 = 0,  hi_J = the number of records.
// The host sizes the loop of an evaluation by the same walk on its copy of the gates (sq_size): R = the most jumps of a
// circuit, and the sweeps of a run = ceil(longest run / kSqOpsPerSweep).
#pragma once
#include <stdint.h>
#include <vector>
#include "vqe_qjump.h"

namespace vqe {

constexpr int kSqOpsPerSweep = 1;      // rotation records applied per read-modify-write sweep of a state

// jpos[j] = the position of the j-th jump record (QJ_JUMP1 / QJ_JUMP2), j < cap; returns the number of jumps.
VQE_HD inline int sq_jump_positions(const QjOp* ops, int nops, int32_t* jpos, int cap) {
  int nj = 0;
  for (int o = 0; o < nops; ++o) {
    const int k = ops[o].kind & 0xff;
    if (k == QJ_JUMP1 || k == QJ_JUMP2) {
      if (nj < cap) jpos[nj] = o;
      ++nj;
    }
  }
  return nj;
}

// The rotation run of round r <= njump: records [*lo, *hi); r < njump: the jump of the round is the record at *hi.
VQE_HD inline void sq_round(const QjOp* ops, int nops, const int32_t* jpos, int njump, int r, int* lo, int* hi) {
  int l = 0;
  if (r > 0) {
    const int j = jpos[r - 1];
    l = j + ((ops[j].kind & 0xff) == QJ_JUMP2 ? 2 : 1);
  }
  *lo = l;
  *hi = r < njump ? jpos[r] : nops;
}

struct SqSize {
  int rounds = 0;      // jump rounds R: the most jumps of a circuit
  int longest = 0;     // the longest rotation run of a circuit
  int sweeps = 0;      // rotation sweeps launched per round
};

// The loop of one evaluation of `batch` circuits (gates[gbeg[b] .. gbeg[b] + gcnt[b])) on n qubits.
inline SqSize sq_size(const GateRec* gates, const int64_t* gbeg, const int32_t* gcnt, int batch, int n, bool slot1, bool slot2) {
  SqSize s;
  std::vector<QjOp> ops;
  std::vector<int32_t> jpos;
  uint32_t xm[32], zm[32], c = 0;
  for (int b = 0; b < batch; ++b) {
    const int G = gcnt[b];
    ops.resize((size_t)2 * G + 1);
    jpos.resize((size_t)G + 1);
    const int nops = qj_compile(gates + gbeg[b], G, n, slot1, slot2, ops.data(), (int)ops.size(), xm, zm, &c);
    const int nj = sq_jump_positions(ops.data(), nops, jpos.data(), (int)jpos.size());
    if (nj > s.rounds) s.rounds = nj;
    for (int r = 0; r <= nj; ++r) {
      int lo, hi;
      sq_round(ops.data(), nops, jpos.data(), nj, r, &lo, &hi);
      if (hi - lo > s.longest) s.longest = hi - lo;
    }
  }
  s.sweeps = (s.longest + kSqOpsPerSweep - 1) / kSqOpsPerSweep;
  return s;
}

}  // namespace vqe
