// CPU check of the unit arrays as the unit loop reads them (tensorrl-qas_amd/csrc/ham_layout.h: unit_arrays): the
// accumulated units of the planned layout followed by the look-ahead trips that the loop only prefetches.  Driven by
// tests/test_unit_padding_cpu.py.
//
//   unit_padding_check TERMS WANT_UNITS
//
// TERMS: "n", then "x z cr ci" per term (the format of ham_layout_check.cpp).  WANT_UNITS: the units the Hamiltonian
// must be held as before any padding (records other than 0).  Prints "units REAL N_UNITS TOTAL" and "ok".
#include "ham_layout.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace vqe;

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

bool zero_bits(double v) { const double z = 0.0; return std::memcmp(&v, &z, 8) == 0; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s TERMS WANT_UNITS\n", argv[0]); return 2; }
  int n = 0;
  FILE* f = std::fopen(argv[1], "r");
  if (!f || std::fscanf(f, "%d", &n) != 1 || n < 1 || n > 13) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  unsigned long long x, z;
  double cr, ci;
  std::vector<uint64_t> xs, zs;
  std::vector<double> coeff;
  while (std::fscanf(f, "%llu %llu %la %la", &x, &z, &cr, &ci) == 4) {
    const int ny = __builtin_popcountll(x & z) & 3;
    xs.push_back(x); zs.push_back(z);
    coeff.push_back(ny == 0 ? cr : ny == 2 ? -cr : ny == 1 ? ci : -ci);
  }
  std::fclose(f);
  const size_t want = (size_t)std::atoi(argv[2]);
  HamHost H;
  CHECK(ham_from_paulis(n, (int)coeff.size(), xs.data(), zs.data(), coeff.data(), H), "mask out of range");
  HamLayout L;
  std::string err;
  CHECK(plan_hamiltonian(H, n, true, 0, 1, true, L, err), "plan_hamiltonian: %s", err.c_str());
  const int lt = geo_lt(n);
  const size_t NT = (size_t)1 << lt;

  // the layout itself: WANT real units, padded with zero units to whole turns
  size_t real = 0;
  for (uint32_t r : L.urec) real += r != 0;
  CHECK(real == want, "%zu units, expected %zu", real, want);
  const size_t turns = (want + kUnitUnroll - 1) / kUnitUnroll;
  CHECK(L.urec.size() == turns * kUnitUnroll, "layout holds %zu units, expected %zu whole turns", L.urec.size(), turns);

  const UnitArrays A = unit_arrays(L, lt);
  const size_t nu = L.urec.size();
  CHECK((size_t)A.n_units == nu, "n_units = %d, the layout has %zu", A.n_units, nu);
  if (!nu) {
    CHECK(A.urec.empty() && A.uaddr.empty() && A.utab.empty(), "a layout without units got look-ahead trips");
    std::printf("units 0 0 0\nok\n");
    return 0;
  }
  // accumulated trips plus two look-ahead trips
  const size_t trips = nu / kUnitTrip, total = nu + 2 * (size_t)kUnitTrip;
  CHECK(kUnitAhead == 2 * kUnitTrip, "kUnitAhead = %d", kUnitAhead);
  CHECK(A.urec.size() == total && A.uaddr.size() == total * NT && A.utab.size() == total * NT,
        "arrays hold %zu records, %zu addresses, %zu values; expected %zu units", A.urec.size(), A.uaddr.size(), A.utab.size(), total);
  // ... the accumulated part exactly the layout's
  CHECK(std::memcmp(A.urec.data(), L.urec.data(), nu * sizeof(uint32_t)) == 0, "records of the accumulated trips changed");
  CHECK(std::memcmp(A.uaddr.data(), L.uaddr.data(), nu * NT * sizeof(uint32_t)) == 0, "addresses of the accumulated trips changed");
  CHECK(std::memcmp(A.utab.data(), L.utab.data(), nu * NT * sizeof(double)) == 0, "table values of the accumulated trips changed");
  // ... the look-ahead part: zero records, zero tables, addresses inside the state
  for (size_t u = nu; u < total; ++u) CHECK(A.urec[u] == 0u, "look-ahead unit %zu has record %u", u, A.urec[u]);
  for (size_t i = nu * NT; i < total * NT; ++i) {
    CHECK(zero_bits(A.utab[i]), "look-ahead table value %zu is not +0.0", i);
    CHECK(A.uaddr[i] == 0u, "look-ahead address %zu is %u", i, A.uaddr[i]);
  }
  // every address of the arrays (both pair members) is a 16-byte slot of the 2^n-amplitude state
  const uint32_t state_bytes = 16u << n;
  for (size_t u = 0; u < total; ++u)
    for (size_t t = 0; t < NT; ++t) {
      const uint32_t a = A.uaddr[((u / kUnitTrip) * NT + t) * kUnitTrip + u % kUnitTrip];
      CHECK((a & 15u) == 0 && a < state_bytes && (a ^ A.urec[u]) < state_bytes, "unit %zu thread %zu: address %u (record %u) outside the state", u, t, a, A.urec[u]);
    }
  // what the loop requests: while it accumulates trip T it loads tables and addresses of trip T + 2 (per thread 32 and
  // 16 bytes at [trip][thread]) and the record of trip T + 1 (16 bytes), by offsets that only step - the last requests
  // must end inside the arrays
  const size_t last_tab = ((trips - 1 + 2) * NT + (NT - 1)) * 32 + 32, last_addr = ((trips - 1 + 2) * NT + (NT - 1)) * 16 + 16;
  const size_t last_rec = (trips - 1 + 1) * 16 + 16;
  CHECK(last_tab <= A.utab.size() * sizeof(double) && last_addr <= A.uaddr.size() * sizeof(uint32_t) && last_rec <= A.urec.size() * sizeof(uint32_t),
        "the loop's last prefetch runs beyond the arrays");
  CHECK(A.utab.size() * sizeof(double) <= 0x7FFFFFFFu, "table offsets beyond 31 bits");
  // the bank-swizzle score reads the real units only: the same with and without the look-ahead trips
  const SwzChoice s0 = choose_bank_swizzle(lt, L.urec, L.uaddr), s1 = choose_bank_swizzle(lt, A.urec, A.uaddr);
  CHECK(s0.swz == s1.swz && s0.mean0 == s1.mean0 && s0.worst0 == s1.worst0 && s0.mean == s1.mean && s0.worst == s1.worst,
        "bank-swizzle score changed with the look-ahead trips: mean %.17g -> %.17g", s0.mean, s1.mean);
  std::printf("units %zu %zu %zu\nok\n", real, nu, total);
  return 0;
}
