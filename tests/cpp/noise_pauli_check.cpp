// noise_pauli_check.cpp - host check of csrc/noise_pauli.h (tests/test_noise_pauli_cpu.py builds it with g++ and
// -fsanitize=address,undefined and runs it as a program): the cumulative table and the branch-free draw.
//   argv[1]: a text file, one table per line: m w_1 ... w_m (m = 0: an empty table), hexadecimal floating point.
// For every table it prints "cum <t> c_1 .. c_m" and, for every u of a grid, "draw <t> <u> <code>", all numbers as
// hexadecimal floating point, so the Python test compares bits with its own restatement of the rule.  The grid: 0, the
// smallest positive double, every threshold with its two neighbouring doubles, the midpoints between consecutive
// thresholds, 1 - 2^-53 and 1.  Here every code is also checked against a search (the smallest k with u < cum_k) and
// the properties of the rule: an entry of width 0 is never selected, the codes do not decrease in u, and u at or past the
// total gives 0.  pauli_weights_ok: NaN, negative, above 1 and a total above 1 + 1e-12 are refused, a total of 1 is not.
// The last line is "ok", or a line "FAIL ..." and exit status 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "noise_pauli.h"

using namespace vqe;

static int fails = 0;
static void check(bool ok, const char* what, int t, double u) {
  if (!ok) { std::printf("FAIL %s table %d u %a\n", what, t, u); ++fails; }
}

static int search_code(double u, const std::vector<double>& cum) {
  for (size_t k = 0; k < cum.size(); ++k) if (u < cum[k]) return (int)k + 1;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: noise_pauli_check tables.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string line;
  int t = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    int m = -1;
    ls >> m;
    if (m < 0) continue;
    std::vector<double> w((size_t)m), cum((size_t)m);
    for (int k = 0; k < m; ++k) { std::string tok; ls >> tok; w[(size_t)k] = std::strtod(tok.c_str(), nullptr); }
    const double total = pauli_cumulate(w.data(), m, cum.data());
    check(total == (m ? cum[(size_t)m - 1] : 0.0), "total", t, total);
    std::printf("cum %d", t);
    for (double c : cum) std::printf(" %a", c);
    std::printf("\n");
    std::vector<double> grid = {0.0, std::numeric_limits<double>::denorm_min(), 1.0 - std::ldexp(1.0, -53), 1.0};
    double prev = 0.0;
    for (double c : cum) {
      grid.push_back(std::nextafter(c, -1.0));
      grid.push_back(c);
      grid.push_back(std::nextafter(c, 2.0));
      grid.push_back(0.5 * (prev + c));
      prev = c;
    }
    for (double u : grid) {
      if (u < 0.0) continue;
      const int code = pauli_code(u, cum.data(), m);
      std::printf("draw %d %a %d\n", t, u, code);
      check(code == search_code(u, cum), "search", t, u);
      check(code >= 0 && code <= m, "range", t, u);
      if (code > 0) check(w[(size_t)code - 1] > 0.0, "zero-width entry selected", t, u);
      if (u >= total) check(code == 0, "past the total", t, u);
      else check(code > 0, "below the total", t, u);
      for (double v : grid) if (v >= u && v < total && u < total) check(pauli_code(v, cum.data(), m) >= code, "monotone", t, u);
    }
    ++t;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double ok1[3] = {0.5, 0.25, 0.25}, bad_nan[3] = {0.1, nan, 0.1}, bad_neg[3] = {0.1, -1e-300, 0.1};
  const double bad_big[3] = {0.0, 1.0 + 1e-9, 0.0}, bad_sum[3] = {0.5, 0.5, 1e-9}, ok_sum[3] = {0.5, 0.5, 1e-13};
  check(pauli_weights_ok(ok1, 3) && pauli_weights_ok(ok_sum, 3) && pauli_weights_ok(ok1, 0), "weights accepted", -1, 0.0);
  check(!pauli_weights_ok(bad_nan, 3) && !pauli_weights_ok(bad_neg, 3) && !pauli_weights_ok(bad_big, 3) && !pauli_weights_ok(bad_sum, 3),
        "weights refused", -1, 0.0);
  std::printf("tables %d\n", t);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
