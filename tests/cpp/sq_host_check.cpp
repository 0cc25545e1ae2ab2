// sq_host_check.cpp - host check of csrc/stream_qjump_host.h (tests/test_stream_kraus_traj_cpu.py builds it with g++ and
// -fsanitize=address,undefined and runs it as a program): the round structure of the streaming path's trajectories.
//  size     sq_size (rounds, longest rotation run, sweeps per round) against a brute-force count over the gate list
//           itself, which shares nothing with qj_compile: a rotation gate is one rotation record, a noise gate whose slot
//           holds a channel is one jump, a CNOT and a noise gate of an identity slot are nothing.  Random batches, both
//           slot settings, and the corner cases by construction: an empty circuit, circuits without noise records, a
//           jump as the first or the last record, a two-qubit jump whose QJ_TAIL is the last record.
//  ranges   sq_jump_positions + sq_round: the runs [lo_r, hi_r) and the jump records between them partition the record
//           list in order; every run holds rotations only; hi_r is a jump record (with its QJ_TAIL behind a QJ_JUMP2).
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "stream_qjump_host.h"

using namespace vqe;

static int fails = 0;
static void check(bool ok, const char* what, long v) {
  if (!ok) { std::printf("FAIL %s %ld\n", what, v); ++fails; }
}

struct Brute { int jumps = 0, longest = 0; };
static Brute brute(const std::vector<GateRec>& g, bool slot1, bool slot2) {
  Brute b;
  int run = 0;
  for (const GateRec& r : g) {
    const bool rot = (r.kind >= G_RX && r.kind <= G_RZ) || (r.kind >= G_RXX && r.kind <= G_RZZ);
    const bool jump = (r.kind == G_DEPOL1 && slot1) || (r.kind == G_DEPOL2 && slot2);
    if (rot) ++run;
    if (jump) { ++b.jumps; b.longest = std::max(b.longest, run); run = 0; }
  }
  b.longest = std::max(b.longest, run);
  return b;
}

static GateRec rot(std::mt19937_64& rng, int n, int* params) {
  const int kinds[6] = {G_RX, G_RY, G_RZ, G_RXX, G_RYY, G_RZZ};
  const int k = kinds[rng() % 6], a = (int)(rng() % n), b = (int)((a + 1 + rng() % (n - 1)) % n);
  return GateRec{k, a, k >= G_RXX ? b : -1, (*params)++};
}
static GateRec noise(std::mt19937_64& rng, int n, bool two) {
  const int a = (int)(rng() % n), b = (int)((a + 1 + rng() % (n - 1)) % n);
  return two ? GateRec{G_DEPOL2, a, b, -1} : GateRec{G_DEPOL1, a, -1, -1};
}
static GateRec cnot(std::mt19937_64& rng, int n) {
  const int a = (int)(rng() % n), b = (int)((a + 1 + rng() % (n - 1)) % n);
  return GateRec{G_CNOT, a, b, -1};
}

static std::vector<GateRec> random_circuit(std::mt19937_64& rng, int n, int G, int noise_pct) {
  std::vector<GateRec> g;
  int params = 0;
  for (int i = 0; i < G; ++i) {
    const int what = (int)(rng() % 100);
    if (what < noise_pct) g.push_back(noise(rng, n, rng() % 2 != 0));
    else if (what < noise_pct + 20) g.push_back(cnot(rng, n));
    else g.push_back(rot(rng, n, &params));
  }
  return g;
}

// the ranges of one circuit; returns its jumps
static int check_ranges(const std::vector<GateRec>& g, int n, bool slot1, bool slot2) {
  std::vector<QjOp> ops(2 * g.size() + 1);
  uint32_t xm[32], zm[32], c = 0;
  const int nops = qj_compile(g.data(), (int)g.size(), n, slot1, slot2, ops.data(), (int)ops.size(), xm, zm, &c);
  check(nops <= (int)ops.size(), "record count", nops);
  std::vector<int32_t> jpos(g.size() + 1, -1);
  const int nj = sq_jump_positions(ops.data(), nops, jpos.data(), (int)jpos.size());
  {      // a short table is not written beyond its end (the sanitizer watches) and the count is the same
    std::vector<int32_t> few((size_t)nj / 2);
    check(sq_jump_positions(ops.data(), nops, few.data(), (int)few.size()) == nj, "short table count", nj);
  }
  check(nj == brute(g, slot1, slot2).jumps, "jumps", nj);
  int next = 0;      // the first record no round has covered yet
  for (int r = 0; r <= nj; ++r) {
    int lo = -1, hi = -1;
    sq_round(ops.data(), nops, jpos.data(), nj, r, &lo, &hi);
    check(lo == next && lo <= hi && hi <= nops, "run follows the previous round", r);
    for (int o = lo; o < hi; ++o) {
      const int k = ops[o].kind & 0xff;
      check(k == G_RX || k == G_RY || k == G_RZ || k == G_RYY, "a run holds rotations", o);
    }
    next = hi;
    if (r < nj) {
      const int k = ops[hi].kind & 0xff;
      check(k == QJ_JUMP1 || k == QJ_JUMP2, "the round's jump", hi);
      if (k == QJ_JUMP2) check(hi + 1 < nops && (ops[hi + 1].kind & 0xff) == QJ_TAIL, "tail record", hi);
      next = hi + (k == QJ_JUMP2 ? 2 : 1);
    }
  }
  check(next == nops, "the rounds cover the list", next);
  return nj;
}

static void check_batch(const std::vector<std::vector<GateRec>>& circuits, int n, bool slot1, bool slot2) {
  std::vector<GateRec> gates;
  std::vector<int64_t> gbeg;
  std::vector<int32_t> gcnt;
  int rounds = 0, longest = 0;
  for (const auto& g : circuits) {
    gbeg.push_back((int64_t)gates.size());
    gcnt.push_back((int32_t)g.size());
    gates.insert(gates.end(), g.begin(), g.end());
    const Brute b = brute(g, slot1, slot2);
    rounds = std::max(rounds, b.jumps);
    longest = std::max(longest, b.longest);
    check_ranges(g, n, slot1, slot2);
  }
  const SqSize s = sq_size(gates.data(), gbeg.data(), gcnt.data(), (int)circuits.size(), n, slot1, slot2);
  check(s.rounds == rounds, "rounds", s.rounds);
  check(s.longest == longest, "longest run", s.longest);
  check(s.sweeps == (longest + kSqOpsPerSweep - 1) / kSqOpsPerSweep, "sweeps", s.sweeps);
  check(s.sweeps * kSqOpsPerSweep >= longest && (s.sweeps == 0 || (s.sweeps - 1) * kSqOpsPerSweep < longest), "sweeps cover the run", s.sweeps);
}

int main() {
  std::mt19937_64 rng(777);
  int batches = 0;
  for (int n : {2, 5, 14})
    for (int rep = 0; rep < 40; ++rep)
      for (int slots = 0; slots < 4; ++slots) {
        std::vector<std::vector<GateRec>> circuits;
        const int B = 1 + (int)(rng() % 4);
        for (int b = 0; b < B; ++b) circuits.push_back(random_circuit(rng, n, (int)(rng() % 40), rep % 4 == 0 ? 0 : 10 + (int)(rng() % 50)));
        check_batch(circuits, n, (slots & 1) != 0, (slots & 2) != 0);
        ++batches;
      }
  // the corner cases by construction
  const int n = 4;
  int params = 0;
  const GateRec r0 = rot(rng, n, &params), r1 = rot(rng, n, &params), r2 = rot(rng, n, &params);
  const GateRec j1 = noise(rng, n, false), j2 = noise(rng, n, true), cx = cnot(rng, n);
  const std::vector<std::vector<GateRec>> corners = {
      {},                          // an empty circuit
      {cx, cx},                    // no records at all
      {r0, cx, r1, r2},            // no noise records: one run, no round
      {j1, r0, r1},                // a jump as the first record
      {r0, r1, j1},                // ... as the last
      {r0, j2},                    // a two-qubit jump whose QJ_TAIL is the last record
      {j2, j1, j2},                // jumps only: every run empty
      {j2},
      {r0, j1, j1, r1, r2, cx, j2, r0}};
  for (int slots = 0; slots < 4; ++slots) {
    for (const auto& g : corners) { check_batch({g}, n, (slots & 1) != 0, (slots & 2) != 0); ++batches; }
    check_batch(corners, n, (slots & 1) != 0, (slots & 2) != 0);
    ++batches;
  }
  {      // the numbers themselves for one of them
    const std::vector<GateRec>& g = corners.back();
    std::vector<int64_t> gbeg{0};
    std::vector<int32_t> gcnt{(int32_t)g.size()};
    const SqSize s = sq_size(g.data(), gbeg.data(), gcnt.data(), 1, n, true, true);
    check(s.rounds == 3 && s.longest == 2 && s.sweeps == (2 + kSqOpsPerSweep - 1) / kSqOpsPerSweep, "corner numbers", s.rounds * 100 + s.longest);
    const SqSize e = sq_size(g.data(), gbeg.data(), gcnt.data(), 0, n, true, true);
    check(e.rounds == 0 && e.longest == 0 && e.sweeps == 0, "empty batch", e.rounds);
  }
  std::printf("batches %d ops_per_sweep %d\n", batches, kSqOpsPerSweep);
  std::printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
