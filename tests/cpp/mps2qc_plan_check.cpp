// CPU check of the fit planner (tensorrl-qas_amd/csrc/mps2qc_plan.h) against the contract k_fit relies on - exactly, no
// tolerance.  Driven by tests/test_mps2qc_plan_cpu.py; takes no arguments, prints "ok" after the last check.
//
// Brickwork circuits n = 2..12, layers = 1..8, and gate sequences with repeated and overlapping pairs, each with the
// half-layer scheme on / off and with / without the two-buffer knob.  What a region must hold is restated here from what
// the kernel touches (k_fit's pointer set-up and loops), not taken from the planner's own size arithmetic.
#include "mps2qc_plan.h"

#include <cstdarg>
#include <cstdlib>
#include <cstring>

using namespace mps2qc;

namespace {

[[noreturn]] void fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::printf("FAIL: ");
  std::vprintf(fmt, ap);
  std::printf("\n");
  va_end(ap);
  std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

std::vector<int32_t> brickwork_sites(int n, int layers) {      // tnqc_ansatze.py:85-95: per layer the even, then the odd bonds
  std::vector<int32_t> s;
  for (int l = 0; l < layers; ++l)
    for (int par = 0; par < 2; ++par)
      for (int i = par; i < n - 1; i += 2) s.push_back(i);
  return s;
}

struct Region { const char* name; size_t off, bytes, align; };

long g_planned = 0, g_refused = 0;

void check_circuit(int n, const std::vector<int32_t>& sites, const char* what) {
  const int G = (int)sites.size();
  char tag[96];
  std::snprintf(tag, sizeof tag, "%s n = %d G = %d", what, n, G);

  // ---- arguments -> lo ----
  std::vector<int> lo;
  std::string err;
  const double dummy = 0.0;
  CHECK(check_fit_args("f", n, 12, G, 1, 1, sites.data(), &dummy, &dummy, lo, err) && err.empty(), "%s: arguments refused: %s", tag, err.c_str());
  CHECK((int)lo.size() == G, "%s: lo has %zu entries", tag, lo.size());
  for (int k = 0; k < G; ++k) CHECK(lo[k] == n - 2 - sites[k], "%s: lo[%d] = %d", tag, k, lo[k]);

  // ---- runs: an ordered partition into maximal runs of pairwise disjoint gates ----
  const std::vector<int> runs = disjoint_runs(lo);
  CHECK(!runs.empty() && runs.size() % 2 == 0, "%s: %zu run entries", tag, runs.size());
  int next = 0, largest = 0;
  for (size_t r = 0; r < runs.size(); r += 2) {
    const int first = runs[r], cnt = runs[r + 1];
    CHECK(first == next && cnt >= 1, "%s: run %zu = [%d, %d] does not continue at gate %d", tag, r / 2, first, cnt, next);
    for (int a = first; a < first + cnt; ++a)
      for (int b = a + 1; b < first + cnt; ++b)
        CHECK(std::abs(sites[a] - sites[b]) >= 2, "%s: gates %d and %d of run %zu share a qubit", tag, a, b, r / 2);
    if (r) {      // maximal: the gate that opened this run did not fit the one before
      bool overlaps = false;
      for (int a = runs[r - 2]; a < first; ++a) overlaps |= std::abs(sites[a] - sites[first]) < 2;
      CHECK(overlaps, "%s: run %zu could have taken gate %d", tag, r / 2 - 1, first);
    }
    next = first + cnt;
    largest = cnt > largest ? cnt : largest;
  }
  CHECK(next == G, "%s: the runs end at gate %d", tag, next);

  // ---- LDS layout ----
  const int NT = threads_per_fit(n), NW = NT / 64, slots = NT / 16 < 16 ? NT / 16 : 16;
  CHECK(NT == (n <= 8 ? 64 : n <= 10 ? 256 : 512), "%s: %d threads per fit", tag, NT);
  const size_t states = 2 * ((size_t)1 << n) * 16, scratch = (size_t)slots * kSlotMats * 16 * 16, red_buf = (size_t)NW * 64 * 8;
  for (int grouped = 0; grouped < 2; ++grouped)
    for (int red2 = 0; red2 < 2; ++red2) {
      FitLds L;
      std::memset(&L, 0xff, sizeof L);
      err.clear();
      const bool ok = plan_fit_lds(n, G, runs, NT, grouped, red2, L, err);
      // everything but the partial buffers, as the planner pads it (the figures of its header comment)
      const size_t rest = states + 2 * (size_t)G * 256 + 256 + (size_t)((G + 1) / 2 * 2) * 8 + (size_t)((G + 3) / 4 * 4) * 4 +
                          (runs.size() + 3) / 4 * 4 * 4 + (states >= scratch ? 0 : scratch);
      const int big = largest > 2 ? largest : 2;      // the kernel double-buffers: never fewer than two
      const int want_slots = grouped && !red2 && rest + big * red_buf <= (size_t)kLdsLimit ? big : 2;
      const size_t want_total = rest + want_slots * red_buf;
      CHECK(ok == (want_total <= (size_t)kLdsLimit), "%s grouped %d red2 %d: planned = %d, the layout needs %zu B", tag, grouped, red2, (int)ok, want_total);
      if (!ok) {
        CHECK(!err.empty(), "%s grouped %d red2 %d: refused without a message", tag, grouped, red2);
        ++g_refused;
        continue;
      }
      ++g_planned;
      CHECK(err.empty(), "%s grouped %d red2 %d: planned with a message: %s", tag, grouped, red2, err.c_str());
      CHECK(L.red_slots == want_slots, "%s grouped %d red2 %d: red_slots = %d, expected %d", tag, grouped, red2, L.red_slots, want_slots);
      CHECK(L.total == want_total && L.total <= (size_t)kLdsLimit, "%s grouped %d red2 %d: total = %zu, expected %zu", tag, grouped, red2, L.total, want_total);
      CHECK((L.off_scratch == 0) == (states >= scratch), "%s grouped %d red2 %d: off_scratch = %d with %zu B of states, %zu B of scratch", tag,
            grouped, red2, L.off_scratch, states, scratch);
      // what the kernel touches in every region
      const Region reg[] = {
          {"psi/phi", 0, states, 16},
          {"U", (size_t)L.off_u, (size_t)G * 256, 16},
          {"E", (size_t)L.off_e, (size_t)G * 256, 16},
          {"red", (size_t)L.off_red, L.red_slots * red_buf, 8},
          {"sc", (size_t)L.off_sc, (size_t)2 * NW * 8, 8},
          {"dn", (size_t)L.off_dn, (size_t)G * 8, 8},
          {"lo", (size_t)L.off_lo, (size_t)G * 4, 4},
          {"grp", (size_t)L.off_grp, runs.size() * 4, 4},
          {"scratch", (size_t)L.off_scratch, scratch, 16},
      };
      const int nreg = sizeof reg / sizeof reg[0];
      for (int a = 0; a < nreg; ++a) {
        CHECK(reg[a].off % reg[a].align == 0, "%s grouped %d red2 %d: %s at %zu is not %zu-byte aligned", tag, grouped, red2, reg[a].name, reg[a].off, reg[a].align);
        CHECK(reg[a].off + reg[a].bytes <= L.total, "%s grouped %d red2 %d: %s ends at %zu, total %zu", tag, grouped, red2, reg[a].name,
              reg[a].off + reg[a].bytes, L.total);
        for (int b = a + 1; b < nreg; ++b) {
          if (a == 0 && b == nreg - 1 && L.off_scratch == 0) continue;      // the permitted overlay
          CHECK(reg[a].off + reg[a].bytes <= reg[b].off || reg[b].off + reg[b].bytes <= reg[a].off, "%s grouped %d red2 %d: %s and %s overlap", tag, grouped,
                red2, reg[a].name, reg[b].name);
        }
      }
    }
}

void check_worked_examples() {
  std::vector<int> lo;
  std::string err;
  const double dummy = 0.0;
  FitLds L;
  // n = 12, one layer: one buffer per gate of the larger half layer
  std::vector<int32_t> s = brickwork_sites(12, 1);
  CHECK(check_fit_args("f", 12, 12, (int)s.size(), 1, 1, s.data(), &dummy, &dummy, lo, err), "example 1: %s", err.c_str());
  std::vector<int> runs = disjoint_runs(lo);
  CHECK(s.size() == 11 && runs == (std::vector<int>{0, 6, 6, 5}), "example 1: runs");
  CHECK(plan_fit_lds(12, 11, runs, 512, true, false, L, err), "example 1: %s", err.c_str());
  CHECK(L.off_u == 131072 && L.off_e == 133888 && L.off_red == 136704 && L.red_slots == 6 && L.off_sc == 161280 && L.off_dn == 161536 &&
            L.off_lo == 161632 && L.off_grp == 161680 && L.off_scratch == 0 && L.total == 161696, "example 1: offsets");
  // four layers: six buffers no longer fit, back to two
  s = brickwork_sites(12, 4);
  CHECK(check_fit_args("f", 12, 12, (int)s.size(), 1, 1, s.data(), &dummy, &dummy, lo, err), "example 2: %s", err.c_str());
  runs = disjoint_runs(lo);
  CHECK(s.size() == 44 && runs.size() == 16, "example 2: runs");
  CHECK(plan_fit_lds(12, 44, runs, 512, true, false, L, err), "example 2: %s", err.c_str());
  CHECK(L.red_slots == 2 && L.total == 162640, "example 2: red_slots %d total %zu", L.red_slots, L.total);
  // six layers: the two gate arrays alone reach 164864 > 163840 beside the two 64-KiB states; refused
  s = brickwork_sites(12, 6);
  CHECK(check_fit_args("f", 12, 12, (int)s.size(), 1, 1, s.data(), &dummy, &dummy, lo, err), "example 3: %s", err.c_str());
  runs = disjoint_runs(lo);
  CHECK(s.size() == 66 && !plan_fit_lds(12, 66, runs, 512, true, false, L, err), "example 3: 66 gates were not refused");
  CHECK(L.off_red == 164864 && L.off_red > kLdsLimit && kLdsLimit == 163840, "example 3: off_red = %d", L.off_red);
  CHECK(err == "mps2qc_fit_brickwork: 66 gates at 12 qubits need 174208 B of LDS (limit 163840)", "example 3: message: %s", err.c_str());
}

void check_arguments() {
  std::vector<int> lo;
  std::string err;
  const double dummy = 0.0;
  const int32_t good[2] = {0, 2}, low[2] = {0, -1}, high[2] = {0, 3};
  CHECK(check_fit_args("fn", 4, 12, 2, 1, 1, good, &dummy, &dummy, lo, err) && lo == (std::vector<int>{2, 0}), "valid arguments refused");
  const char* bad = "fn: bad argument (2 <= n <= 12, G, batch, max_iter >= 1)";
  CHECK(!check_fit_args("fn", 1, 12, 2, 1, 1, good, &dummy, &dummy, lo, err) && err == bad, "n = 1: %s", err.c_str());
  CHECK(!check_fit_args("fn", 13, 12, 2, 1, 1, good, &dummy, &dummy, lo, err) && err == bad, "n = 13: %s", err.c_str());
  CHECK(!check_fit_args("fn", 4, 12, 0, 1, 1, good, &dummy, &dummy, lo, err) && err == bad, "G = 0");
  CHECK(!check_fit_args("fn", 4, 12, 2, 0, 1, good, &dummy, &dummy, lo, err) && err == bad, "batch = 0");
  CHECK(!check_fit_args("fn", 4, 12, 2, 1, 0, good, &dummy, &dummy, lo, err) && err == bad, "max_iter = 0");
  CHECK(!check_fit_args("fn", 4, 12, 2, 1, 1, nullptr, &dummy, &dummy, lo, err) && err == bad, "sites = NULL");
  CHECK(!check_fit_args("fn", 4, 12, 2, 1, 1, good, nullptr, &dummy, lo, err) && err == bad, "target = NULL");
  CHECK(!check_fit_args("fn", 4, 12, 2, 1, 1, good, &dummy, nullptr, lo, err) && err == bad, "init_gates = NULL");
  CHECK(!check_fit_args("fn", 4, 12, 2, 1, 1, low, &dummy, &dummy, lo, err) && err == "fn: gate 1 on sites (-1,0) outside the register", "site -1: %s", err.c_str());
  CHECK(!check_fit_args("fn", 4, 12, 2, 1, 1, high, &dummy, &dummy, lo, err) && err == "fn: gate 1 on sites (3,4) outside the register", "site 3: %s", err.c_str());
  CHECK(check_fit_args("fn", 26, 26, 2, 1, 1, good, &dummy, &dummy, lo, err) && lo == (std::vector<int>{24, 22}), "n = 26 refused");
}

void check_lr_schedule() {
  const double lr = 3e-3, b1 = 0.9, b2 = 0.999;
  for (int it : {0, 1, 2, 7, 59, 1999}) {
    CHECK(same_bits(lr_schedule(lr, b1, b2, true, it), lr_schedule(lr, b1, b2, true, 0)), "frozen schedule moves at it = %d", it);
    const double t = (double)(it + 1);
    CHECK(same_bits(lr_schedule(lr, b1, b2, false, it), lr * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t))), "schedule at it = %d", it);
  }
  CHECK(same_bits(lr_schedule(lr, b1, b2, true, 5), lr_schedule(lr, b1, b2, false, 0)), "frozen is not step 1");
}

}  // namespace

int main() {
  check_arguments();
  check_worked_examples();
  check_lr_schedule();
  for (int n = 2; n <= 12; ++n)
    for (int layers = 1; layers <= 8; ++layers) check_circuit(n, brickwork_sites(n, layers), "brickwork");
  for (int n : {4, 6, 12}) {
    const std::vector<std::vector<int32_t>> seqs = {
        {0, 1, 2},                                  // a staircase: every run has one gate
        {n - 2},                                    // a single gate
        {n - 2, 0, 2, 1, n - 3, 0},                 // paired gates far apart, overlaps
        {0, n - 2, 2, 1, 2, 0},
        {0, 0, 0},                                  // the same pair again and again
        {1, 1, n - 2, n - 2, 1, 0, 2, 0, 2},
    };
    for (const auto& s : seqs) check_circuit(n, s, "sequence");
  }
  std::printf("planned %ld refused %ld\nok\n", g_planned, g_refused);
  return 0;
}
