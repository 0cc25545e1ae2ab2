// CPU check of the Hamiltonian layout planner (tensorrl-qas_amd/csrc/ham_layout.h) against the contract the energy
// kernels rely on - exactly, no tolerance.  Driven by tests/test_ham_layout_cpu.py.
//
//   ham_layout_check TERMS UNITS_ON WORLD [WORLD ...]
//
// TERMS: "n", then "x z cr ci" per term (c i^{#Y} split into real and imaginary part, hex floats).  For every WORLD the
// layouts and the gradient tables of the shards rank = 0..WORLD-1 are planned and checked; one line per shard
// "shard WORLD RANK groups padding units swz mean0 mean" is printed for the caller.  Every expected value is
// recomputed here from the term list and the definitions (HamLayout's comments), not with the planner's routines.
#include "ham_layout.h"

#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

using namespace vqe;

namespace {

int g_n = 0;
std::vector<uint32_t> g_x, g_z;      // the input terms
std::vector<double> g_cr, g_ci;
std::vector<uint32_t> g_group_x;     // X masks in order of first appearance
std::map<uint32_t, std::vector<int>> g_terms_of;   // X mask -> its terms, input order

[[noreturn]] void fail(int world, int rank, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
void fail(int world, int rank, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::printf("FAIL world %d rank %d: ", world, rank);
  std::vprintf(fmt, ap);
  std::printf("\n");
  va_end(ap);
  std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) fail(world, rank, __VA_ARGS__); } while (0)

int parity(uint32_t v) { return __builtin_popcount(v) & 1; }
int hibit(uint32_t x) { int b = -1; while (x) { ++b; x >>= 1; } return b; }
uint32_t ins0(uint32_t q, int b) { const uint32_t low = q & ((1u << b) - 1u); return ((q - low) << 1) | low; }
bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// x' = M x, z' = M^-T z, x = M^-1 x' - from the rows of M and the columns of M^-1 as the layout states them
uint32_t map_x(const IndexMap& m, uint32_t x) { uint32_t r = 0; for (int i = 0; i < g_n; ++i) r |= (uint32_t)parity(m.row[i] & x) << i; return r; }
uint32_t map_z(const IndexMap& m, uint32_t z) { uint32_t r = 0; for (int i = 0; i < g_n; ++i) r |= (uint32_t)parity(m.inv_col[i] & z) << i; return r; }
uint32_t unmap_x(const IndexMap& m, uint32_t xp) { uint32_t r = 0; for (int i = 0; i < g_n; ++i) if ((xp >> i) & 1u) r ^= m.inv_col[i]; return r; }

// sum_k c_k (-1)^{popc(p & z_k)} factor over the terms of X-mask group x, input order; z_k mapped by `m` when given
double direct(uint32_t x, const IndexMap* m, uint32_t p, double factor, const std::vector<double>& c) {
  double acc = 0.0;
  for (int k : g_terms_of[x]) {
    const uint32_t z = m ? map_z(*m, g_z[k]) : g_z[k];
    acc += (parity(p & z) ? -1.0 : 1.0) * factor * c[k];
  }
  return acc;
}
bool has_im(uint32_t x) { for (int k : g_terms_of[x]) if (g_ci[k] != 0.0) return true; return false; }

// one shard's layout; returns the X masks (input space) it holds
std::set<uint32_t> check_shard(const HamHost& H, bool lds_path, bool units_on, int world, int rank, std::map<uint32_t, int>& seen) {
  const int n = g_n;
  HamLayout L;
  std::string err;
  CHECK(plan_hamiltonian(H, n, lds_path, rank, world, units_on, L, err), "plan_hamiltonian: %s", err.c_str());
  const IndexMap& M = L.im;
  const int lt = geo_lt(n), pd = energy_pd(n);
  const bool reg_path = lds_path && n >= kRegMinQubits;
  const size_t dim = (size_t)1 << n, NT = (size_t)1 << lt;
  std::set<uint32_t> mine;

  // ---- shape: M, S, mrow ----
  CHECK(M.n == n, "index map has n = %d", M.n);
  for (int j = 0; j < n; ++j)
    CHECK(unmap_x(M, map_x(M, 1u << j)) == (1u << j), "inv_col is not the inverse of M (column %d)", j);
  auto code = [&](uint32_t v) { return (uint32_t)((L.swz >> (4 * v)) & 15u); };
  for (uint32_t a = 0; a < 16; ++a) for (uint32_t b = 0; b < 16; ++b)
    CHECK(code(a ^ b) == (code(a) ^ code(b)), "swz is not GF(2)-linear at (%u, %u)", a, b);
  for (uint32_t p = 0; p < dim && p < (1u << 16); ++p) {
    const uint32_t slot = swz_slot(L.swz, map_x(M, p));
    for (int i = 0; i < 16; ++i)
      CHECK(parity(L.mrow[i] & p) == (int)((slot >> i) & 1u), "mrow[%d] is not row %d of S M (p = %u)", i, i, p);
  }
  CHECK(L.mean <= L.mean0, "bank score got worse: mean %.17g > mean0 %.17g", L.mean, L.mean0);
  if (!L.swz) CHECK(L.mean == L.mean0 && L.worst == L.worst0, "identity swizzle with scores that differ");
  if (!(reg_path && !L.urec.empty() && L.gx.size() == (size_t)(L.has_diag + L.n_cls)))
    CHECK(L.swz == 0, "swz = %" PRIx64 " where the layout must keep S = I", L.swz);

  // ---- group list ----
  const size_t G = L.gx.size();
  CHECK(L.tab_r.size() == G && L.tab_i.size() == G && L.term_off.size() == G + 1 && L.term_off[0] == 0, "group list array sizes");
  CHECK(L.term_z.size() == (size_t)L.term_off[G] && L.term_cr.size() == L.term_z.size() && L.term_ci.size() == L.term_z.size(), "term array sizes");
  if (lds_path) {
    CHECK(L.n_cls % pd == 0 && (L.n_real - L.n_cls) % pd == 0 && L.n_cls >= 0 && L.n_real >= L.n_cls,
          "n_cls = %d, n_real = %d are not padded to multiples of %d", L.n_cls, L.n_real, pd);
    CHECK((size_t)(L.has_diag + L.n_real) <= G && (L.has_diag == 0 || L.has_diag == 1), "has_diag / n_real out of range");
    CHECK(reg_path || L.n_cls == 0, "class groups below the register path");
  } else {
    CHECK(L.has_diag == 0 && L.n_real == 0 && L.n_cls == 0 && L.tables.empty() && L.urec.empty(), "streaming path: term arrays only");
  }
  int n_pad = 0, prev_section = -1, prev_top = 99;
  size_t next_table = 0;
  for (size_t e = 0; e < G; ++e) {
    const uint32_t xp = L.gx[e];
    const int t0 = L.term_off[e], t1 = L.term_off[e + 1];
    const bool padding = t1 == t0;
    // section by position: 0 diagonal, 1 class, 2 plain real, 3 imaginary
    const int section = !lds_path ? 0 : e < (size_t)L.has_diag ? 0 : e < (size_t)(L.has_diag + L.n_cls) ? 1 : e < (size_t)(L.has_diag + L.n_real) ? 2 : 3;
    if (lds_path) {
      if (section != prev_section) prev_top = 99;
      CHECK(section >= prev_section && hibit(xp) <= prev_top, "entry %zu breaks the section / top-bit order", e);
      prev_section = section;
      prev_top = hibit(xp);
    }
    if (padding) {
      ++n_pad;
      CHECK(lds_path && (section == 1 || section == 2), "padding entry %zu outside the real sections", e);
      CHECK(xp == (section == 1 ? 1u << lt : 1u) && L.tab_i[e] == -1 && (size_t)L.tab_r[e] == next_table, "padding entry %zu: mask / table offsets", e);
      for (size_t q = 0; q < dim / 2; ++q) CHECK(same_bits(L.tables[next_table + q], 0.0), "padding entry %zu has a non-zero table", e);
      next_table += dim / 2;
      continue;
    }
    const uint32_t x = unmap_x(M, xp);
    CHECK(map_x(M, x) == xp && g_terms_of.count(x), "entry %zu: x' = %u is not the image of an input group", e, xp);
    CHECK(mine.insert(x).second, "group x = %u twice in the group list", x);
    const std::vector<int>& terms = g_terms_of[x];
    CHECK((size_t)(t1 - t0) == terms.size(), "entry %zu: %d terms, input has %zu", e, t1 - t0, terms.size());
    for (size_t i = 0; i < terms.size(); ++i) {
      const int k = terms[i];
      CHECK(L.term_z[t0 + i] == map_z(M, g_z[k]) && same_bits(L.term_cr[t0 + i], g_cr[k]) && same_bits(L.term_ci[t0 + i], g_ci[k]),
            "entry %zu: term %zu differs from input term %d", e, i, k);
    }
    const bool im = has_im(x);
    if (!lds_path) {
      CHECK(L.tab_r[e] == 0 && L.tab_i[e] == (im ? 0 : -1), "entry %zu: streaming-path table markers", e);
      continue;
    }
    const int want = im ? 3 : xp == 0 ? 0 : (reg_path && (xp >> lt)) ? 1 : 2;
    CHECK(section == want, "entry %zu (x' = %u) sits in section %d, belongs to %d", e, xp, section, want);
    const size_t len = xp == 0 ? dim : dim / 2;
    CHECK((size_t)L.tab_r[e] == next_table && L.tab_i[e] == (im ? (int32_t)(next_table + len) : -1), "entry %zu: table offsets", e);
    next_table += im ? 2 * len : len;
    CHECK(next_table <= L.tables.size(), "entry %zu: table beyond the end", e);
    const double factor = xp == 0 ? 1.0 : 2.0;
    for (size_t q = 0; q < len; ++q) {
      uint32_t p;
      if (xp == 0) p = (uint32_t)q;
      else if (section == 1) {      // [j/2][tid][j&1]
        const uint32_t tid = (uint32_t)(q >> 1) & (uint32_t)(NT - 1), j = (uint32_t)((q >> (lt + 1)) << 1) | (uint32_t)(q & 1);
        p = tid | (ins0(j, hibit(xp) - lt) << lt);
      } else p = ins0((uint32_t)q, hibit(xp));
      CHECK(same_bits(L.tables[L.tab_r[e] + q], direct(x, &M, p, factor, g_cr)), "entry %zu (x' = %u): real table slot %zu", e, xp, q);
      if (im) CHECK(same_bits(L.tables[L.tab_i[e] + q], direct(x, &M, p, factor, g_ci)), "entry %zu (x' = %u): imaginary table slot %zu", e, xp, q);
    }
  }
  CHECK(next_table == L.tables.size(), "tables hold %zu doubles, the group list accounts for %zu", L.tables.size(), next_table);
  if (lds_path && G) CHECK(L.has_diag == (L.gx[0] == 0 && L.term_off[1] > 0), "has_diag does not match entry 0");

  // ---- units ----
  const size_t U = L.urec.size();
  CHECK(U % kUnitUnroll == 0 && L.uaddr.size() == U * NT && L.utab.size() == U * NT, "unit arrays: %zu units, %zu addresses, %zu values", U, L.uaddr.size(), L.utab.size());
  CHECK(U == 0 || (units_on && lds_path && n >= kUnitMinQubits && n - 1 - lt >= 1), "units outside the unit path's range");
  std::map<uint32_t, std::vector<uint8_t>> cover;      // x -> per canonical index: (unit, thread) entries that hold it
  for (size_t u = 0; u < U; ++u) {
    const uint32_t rec = L.urec[u];
    uint32_t x = 0, xp = 0;
    double bound = 0.0;
    if (rec) {
      CHECK((rec & 15u) == 0, "unit %zu: urec is not a 16-byte distance", u);
      xp = swz_slot(L.swz, rec >> 4);
      x = unmap_x(M, xp);
      CHECK(xp && map_x(M, x) == xp && g_terms_of.count(x) && !has_im(x), "unit %zu: x' = %u is not the image of a real input group", u, xp);
      CHECK(!mine.count(x) || cover.count(x), "group x = %u in the group list and in the unit list", x);
      mine.insert(x);
      if (!cover.count(x)) cover[x].assign(dim, 0);
      double scale = 0.0;
      for (int k : g_terms_of[x]) scale += std::fabs(2.0 * g_cr[k]);
      bound = kUnitZeroTol * scale;
    }
    for (size_t t = 0; t < NT; ++t) {
      const size_t at = ((u / kUnitTrip) * NT + t) * kUnitTrip + u % kUnitTrip;
      if (!rec) {
        CHECK(L.uaddr[at] == 0 && same_bits(L.utab[at], 0.0), "padding unit %zu thread %zu is not all zero", u, t);
        continue;
      }
      CHECK((L.uaddr[at] & 15u) == 0, "unit %zu thread %zu: uaddr is not a 16-byte address", u, t);
      const uint32_t p0 = swz_slot(L.swz, L.uaddr[at] >> 4);
      CHECK(p0 < dim && !((p0 >> hibit(xp)) & 1u), "unit %zu thread %zu: %u is not a selector-0 index", u, t, p0);
      const double d = direct(x, &M, p0, 2.0, g_cr);
      CHECK(same_bits(L.utab[at], std::fabs(d) > bound ? d : 0.0), "unit %zu thread %zu (x' = %u, p0 = %u): table value", u, t, xp, p0);
      CHECK(++cover[x][p0] == 1, "pair p0 = %u of group x' = %u held twice", p0, xp);
    }
  }
  for (const auto& kv : cover) {
    const uint32_t x = kv.first, xp = map_x(M, x);
    double scale = 0.0;
    for (int k : g_terms_of[x]) scale += std::fabs(2.0 * g_cr[k]);
    for (uint32_t p0 = 0; p0 < dim; ++p0)
      if (!((p0 >> hibit(xp)) & 1u) && std::fabs(direct(x, &M, p0, 2.0, g_cr)) > kUnitZeroTol * scale)
        CHECK(kv.second[p0] == 1, "non-zero pair p0 = %u of unit group x' = %u is in no unit", p0, xp);
  }
  for (uint32_t x : mine) CHECK(++seen[x] == 1, "group x = %u in more than one shard", x);

  // ---- gradient tables: the shard's groups in input order, logical index ----
  if (lds_path) {
    GradTables T;
    plan_grad_tables(H, n, lds_path, rank, world, T);
    std::vector<uint32_t> order;
    for (uint32_t x : g_group_x) if (mine.count(x)) order.push_back(x);
    CHECK(T.gx == order && T.off.size() == order.size() && T.cplx.size() == order.size(), "gradient tables: group list differs from the shard's");
    size_t at = 0;
    for (size_t e = 0; e < order.size(); ++e) {
      const uint32_t x = order[e];
      const bool im = has_im(x);
      const size_t len = x == 0 ? dim : dim / 2;
      CHECK((size_t)T.off[e] == at && T.cplx[e] == (im ? 1 : 0), "gradient group %zu: offset / complex flag", e);
      at += (im ? 2 : 1) * len;
      CHECK(at <= T.tab.size(), "gradient group %zu: table beyond the end", e);
      for (size_t q = 0; q < len; ++q) {
        const uint32_t p = x == 0 ? (uint32_t)q : ins0((uint32_t)q, hibit(x));
        const double* t = T.tab.data() + T.off[e] + (im ? 2 * q : q);
        CHECK(same_bits(t[0], direct(x, nullptr, p, 1.0, g_cr)), "gradient group %zu slot %zu: real part", e, q);
        if (im) CHECK(same_bits(t[1], direct(x, nullptr, p, 1.0, g_ci)), "gradient group %zu slot %zu: imaginary part", e, q);
      }
    }
    CHECK(at == T.tab.size(), "gradient tables hold %zu doubles, the groups account for %zu", T.tab.size(), at);
  }
  std::printf("shard %d %d %zu %d %zu %" PRIx64 " %.17g %.17g\n", world, rank, G - n_pad, n_pad, U, L.swz, L.mean0, L.mean);
  return mine;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s TERMS UNITS_ON WORLD [WORLD ...]\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f || std::fscanf(f, "%d", &g_n) != 1 || g_n < 1 || g_n > 30) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  unsigned long long x, z;
  double cr, ci;
  std::vector<uint64_t> xs, zs;
  std::vector<double> coeff;
  while (std::fscanf(f, "%llu %llu %la %la", &x, &z, &cr, &ci) == 4) {
    if (!g_terms_of.count((uint32_t)x)) g_group_x.push_back((uint32_t)x);
    g_terms_of[(uint32_t)x].push_back((int)g_x.size());
    g_x.push_back((uint32_t)x); g_z.push_back((uint32_t)z); g_cr.push_back(cr); g_ci.push_back(ci);
    // the library's entry point takes the coefficient of the Pauli string: divide c i^{#Y} by i^{#Y}
    const int ny = __builtin_popcountll(x & z) & 3;
    xs.push_back(x); zs.push_back(z);
    coeff.push_back(ny == 0 ? cr : ny == 2 ? -cr : ny == 1 ? ci : -ci);
  }
  std::fclose(f);
  HamHost H;
  if (!ham_from_paulis(g_n, (int)coeff.size(), xs.data(), zs.data(), coeff.data(), H)) { std::printf("FAIL: mask out of range\n"); return 1; }
  for (size_t k = 0; k < coeff.size(); ++k)
    if (!same_bits(H.hcr[k], g_cr[k]) || !same_bits(H.hci[k], g_ci[k])) { std::printf("FAIL: term %zu: c i^{#Y} differs from the input\n", k); return 1; }
  const bool lds_path = g_n <= 13, units_on = std::atoi(argv[2]) != 0;
  for (int a = 3; a < argc; ++a) {
    const int world = std::atoi(argv[a]);
    std::map<uint32_t, int> seen;
    for (int rank = 0; rank < world; ++rank) check_shard(H, lds_path, units_on, world, rank, seen);
    for (uint32_t gx : g_group_x)
      if (seen[gx] != 1) { std::printf("FAIL world %d: group x = %u is in %d shards\n", world, gx, seen[gx]); return 1; }
  }
  std::printf("ok\n");
  return 0;
}
