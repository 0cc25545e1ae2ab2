// ham_layout.h - the Hamiltonian layout planner: from the grouped Pauli sum (HamHost) to the arrays that the energy
// kernels read (HamLayout) and the table set of the adjoint kernel (GradTables).  Host only - integer and double
// arithmetic on std::vector, no HIP - so that the planner / kernel contract written down on HamLayout is checked
// without a GPU (tests/cpp/ham_layout_check.cpp).  vqe_api.hip uploads what this file plans.
#pragma once
#include "vqe_geo.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

namespace vqe {

// H = sum_k c_k P(x_k, z_k), P|i> = i^{#Y} (-1)^{popc(i & z)} |i ^ x>, grouped by X mask in order of first appearance
struct HamHost {
  std::vector<uint32_t> gx_all;                 // X mask of group g
  std::vector<std::vector<int>> group_terms;    // its terms, in input order
  std::vector<uint64_t> hx, hz;                 // [n_terms]
  std::vector<double> hcr, hci;                 // [n_terms] c_k i^{#Y}: real and imaginary part
  bool group_has_im(int g) const {
    for (int k : group_terms[g]) if (hci[k] != 0.0) return true;
    return false;
  }
};

// false: a mask uses a qubit >= n
inline bool ham_from_paulis(int n, int n_terms, const uint64_t* xmask, const uint64_t* zmask, const double* coeff, HamHost& H) {
  const uint64_t lim = n >= 64 ? ~0ull : (((uint64_t)1 << n) - 1);
  H.hx.assign(xmask, xmask + n_terms);
  H.hz.assign(zmask, zmask + n_terms);
  H.hcr.assign(n_terms, 0.0);
  H.hci.assign(n_terms, 0.0);
  std::map<uint32_t, int> index;
  H.gx_all.clear();
  H.group_terms.clear();
  for (int k = 0; k < n_terms; ++k) {
    if ((xmask[k] | zmask[k]) & ~lim) return false;
    const int ny = __builtin_popcountll(xmask[k] & zmask[k]) & 3;  // i^{#Y}
    const double w = coeff[k];
    H.hcr[k] = ny == 0 ? w : (ny == 2 ? -w : 0.0);
    H.hci[k] = ny == 1 ? w : (ny == 3 ? -w : 0.0);
    const uint32_t x = (uint32_t)xmask[k];
    auto it = index.find(x);
    if (it == index.end()) {
      it = index.emplace(x, (int)H.gx_all.size()).first;
      H.gx_all.push_back(x);
      H.group_terms.emplace_back();
    }
    H.group_terms[it->second].push_back(k);
  }
  return true;
}

// Pauli-term sharding: greedy bin packing of X-mask groups over ranks by cost (table length
// on the LDS path, partner sweep + terms on the streaming path); deterministic, so every
// rank computes the same partition.
inline std::vector<int> assign_groups(const std::vector<uint32_t>& gx, const std::vector<std::vector<int>>& terms,
                                      bool lds_path, int world) {
  std::vector<int> order(gx.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  auto cost = [&](int g) -> double {
    return lds_path ? (gx[g] == 0 ? 2.0 : 1.0) : 1.0 + 0.25 * (double)terms[g].size();
  };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost(a) > cost(b); });
  std::vector<double> load(world, 0.0);
  std::vector<int> owner(gx.size(), 0);
  for (int g : order) {
    int best = 0;
    for (int r = 1; r < world; ++r) if (load[r] < load[best]) best = r;
    load[best] += cost(g);
    owner[g] = best;
  }
  return owner;
}

// the groups of shard `rank`, ascending
inline std::vector<int> shard_groups(const HamHost& H, bool lds_path, int rank, int world) {
  const std::vector<int> owner = assign_groups(H.gx_all, H.group_terms, lds_path, world);
  std::vector<int> mine;
  for (size_t g = 0; g < owner.size(); ++g) if (owner[g] == rank) mine.push_back((int)g);
  return mine;
}

inline int top_bit(uint32_t x) { return x ? 31 - __builtin_clz(x) : -1; }
// q with a 0 inserted at position `bit`: the pair representative (selector bit clear) of pair number q
inline uint32_t insert0(uint32_t q, int bit) { return ((q >> bit) << (bit + 1)) | (q & ((1u << bit) - 1u)); }

// One term's share of a sign-sum table: t[stride q] += (-1)^{popc(rep[q] & z)} factor c.  The callers add the terms of
// a group in the order of group_terms[g]; table values are compared bit for bit, so that order is part of the layout.
inline void add_sign_term(double* t, size_t stride, const std::vector<uint32_t>& rep, uint32_t z, double factor, double c) {
  for (size_t q = 0; q < rep.size(); ++q) {
    const double sgn = ((__builtin_popcount(rep[q] & z) & 1) ? -1.0 : 1.0) * factor;
    t[stride * q] += sgn * c;
  }
}

inline std::vector<uint32_t> pair_reps(int n, int sel) {
  std::vector<uint32_t> rep((size_t)1 << (n - 1));
  for (size_t q = 0; q < rep.size(); ++q) rep[q] = insert0((uint32_t)q, sel);
  return rep;
}

// ---- canonical index map of the register path -----------------------------------------------
// p' = M p over GF(2).  The top R rows of M are functionals chosen greedily so that as many X
// masks as possible have a non-zero image in the register bits (every one of them in the
// molecular Hamiltonians tried); the lower rows complete M to an invertible matrix with unit
// vectors.  Pauli masks transform as x' = M x, z' = M^-T z.
struct IndexMap {
  int n = 0;
  uint32_t row[32] = {0};      // rows of M (identity beyond the register path's n <= 13)
  uint32_t inv_col[32] = {0};  // columns of M^-1 (as bit masks over its rows)
  uint32_t map_x(uint32_t x) const {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= (uint32_t)(__builtin_popcount(row[i] & x) & 1) << i;
    return r;
  }
  uint32_t map_z(uint32_t z) const {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= (uint32_t)(__builtin_popcount(inv_col[i] & z) & 1) << i;
    return r;
  }
};

inline IndexMap identity_map(int n) {
  IndexMap m;
  m.n = n;
  for (int i = 0; i < n; ++i) m.row[i] = m.inv_col[i] = 1u << i;
  return m;
}

// M^-1 by Gauss-Jordan on [M | I] (rows as bit masks) -> inv_col
inline void finish_inverse(IndexMap& m) {
  const int n = m.n;
  uint32_t a[32], inv[32];
  for (int i = 0; i < n; ++i) { a[i] = m.row[i]; inv[i] = 1u << i; }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    while (piv < n && !((a[piv] >> c) & 1u)) ++piv;
    std::swap(a[c], a[piv]);
    std::swap(inv[c], inv[piv]);
    for (int r = 0; r < n; ++r)
      if (r != c && ((a[r] >> c) & 1u)) { a[r] ^= a[c]; inv[r] ^= inv[c]; }
  }
  for (int i = 0; i < n; ++i) {
    uint32_t col = 0;
    for (int j = 0; j < n; ++j) col |= ((inv[j] >> i) & 1u) << j;
    m.inv_col[i] = col;
  }
}

inline IndexMap choose_index_map(int n, int lt, const std::vector<uint32_t>& xs) {
  IndexMap m;
  m.n = n;
  const int R = n - lt;
  std::vector<uint32_t> rem(xs), rows;     // masks not yet hit / chosen functionals (any order)
  uint32_t ech[32] = {0};                  // echelon basis of the chosen rows, by highest bit
  auto independent = [&](uint32_t v) {
    for (int bit = n - 1; bit >= 0 && v; --bit)
      if (((v >> bit) & 1u) && ech[bit]) v ^= ech[bit];
    return v;
  };
  auto add_row = [&](uint32_t f) {
    const uint32_t red = independent(f);
    ech[top_bit(red)] = red;
    rows.push_back(f);
  };
  for (int i = 0; i < R; ++i) {
    uint32_t best = 0;
    int best_hits = -1;
    if (!rem.empty()) {
      for (uint32_t f = 1; f < (1u << n); ++f) {
        int hits = 0;
        for (uint32_t x : rem) hits += __builtin_popcount(f & x) & 1;
        if (hits > best_hits && independent(f)) { best_hits = hits; best = f; }
      }
    }
    if (best_hits <= 0) {   // nothing left to hit: any independent unit functional
      for (int bit = n - 1; bit >= 0; --bit) if (independent(1u << bit)) { best = 1u << bit; break; }
    }
    add_row(best);
    std::vector<uint32_t> keep;
    for (uint32_t x : rem) if (!(__builtin_popcount(best & x) & 1)) keep.push_back(x);
    rem.swap(keep);
  }
  for (int i = 0; i < R; ++i) m.row[lt + i] = rows[i];
  int filled = 0;
  for (int bit = 0; bit < n && filled < lt; ++bit)
    if (independent(1u << bit)) { add_row(1u << bit); m.row[filled++] = 1u << bit; }
  finish_inverse(m);
  return m;
}

// ---- unit path: X-mask groups with mostly-zero sign-sum tables -------------------------------------
// The sign-sum table D_x(p) = sum_k c_k (-1)^{popc(p & z_k)} of a fermionic excitation operator vanishes EXACTLY on
// every pair {p, p^x} whose occupation pattern the operator does not connect (a hopping pair XZ..ZX + YZ..ZY acts on
// 01 <-> 10 only, a double-excitation octet on one pattern pair in eight): 76 % of the entries of the bench
// Hamiltonian, 69 % of the shipped H2O one.  A group is cut into sub-cubes of NT pairs (fix F = n-1-LT index bits
// besides the selector bit); only sub-cubes on which D does not vanish become *units* (HamLayout::urec).
// Entries below kUnitZeroTol x sum_k |c_k| count as zero (vqe_geo.h).

// a permutation of the qubits as canonical index map: position lt.. (the register bits of the class path) cover
// the masks of the dense groups, the other qubits are placed by how often they are a fixed / selector bit of a
// unit - the most frequent ones highest, so that the lowest index bits (consecutive lanes, LDS banks) stay free
inline IndexMap choose_permutation(int n, int lt, const std::vector<uint32_t>& dense_xs, const std::vector<int>& hole_freq) {
  IndexMap m;
  m.n = n;
  std::vector<int> at(n, -1);            // qubit at canonical position i
  std::vector<bool> used(n, false);
  std::vector<uint32_t> rem(dense_xs);
  for (int pos = n - 1; pos >= 0; --pos) {
    int best = -1;
    if (pos >= lt && !rem.empty()) {
      int best_hits = 0;
      for (int q = 0; q < n; ++q) {
        if (used[q]) continue;
        int hits = 0;
        for (uint32_t x : rem) hits += (x >> q) & 1u;
        if (hits > best_hits) { best_hits = hits; best = q; }
      }
      if (best >= 0) {
        std::vector<uint32_t> keep;
        for (uint32_t x : rem) if (!((x >> best) & 1u)) keep.push_back(x);
        rem.swap(keep);
      }
    }
    if (best < 0)
      for (int q = n - 1; q >= 0; --q)
        if (!used[q] && (best < 0 || hole_freq[q] > hole_freq[best])) best = q;
    used[best] = true;
    at[pos] = best;
  }
  for (int i = 0; i < n; ++i) m.row[i] = m.inv_col[i] = 1u << at[i];
  return m;
}

// sign-sum table of a real group over pair representatives p0 = insert0(q, sel) in the index space of `im`
// (factor 2 of the pair symmetry included, as in the pair tables of the group lists), and its active pairs: the
// representatives whose entry is above the zero bound kUnitZeroTol * scale, scale = sum_k |2 c_k|
inline void pair_table(const HamHost& H, int g, const IndexMap& im, int n, int sel, std::vector<double>& D,
                       double* scale, std::vector<uint32_t>& act) {
  const std::vector<uint32_t> rep = pair_reps(n, sel);
  D.assign(rep.size(), 0.0);
  *scale = 0.0;
  for (int k : H.group_terms[g]) {
    const double c = 2.0 * H.hcr[k];
    *scale += std::fabs(c);
    add_sign_term(D.data(), 1, rep, im.map_z((uint32_t)H.hz[k]), 1.0, c);
  }
  act.clear();
  for (size_t q = 0; q < D.size(); ++q) if (std::fabs(D[q]) > kUnitZeroTol * *scale) act.push_back(rep[q]);
}

// Fixed bits of a group's units: greedily the index bits (not the selector) on which the active pairs agree most;
// stops when no bit helps any more (every remaining one doubles the number of active patterns).  Returns the
// number of active patterns on `fixed`; the units of the group are patterns x 2^(F - |fixed|) (filler bits).
inline int choose_fixed_bits(int n, int sel, int F, const std::vector<uint32_t>& act, std::vector<int>& fixed) {
  fixed.clear();
  if (act.empty()) return 0;
  int patterns = 1;
  auto count = [&](int extra) {
    uint32_t seen = 0;
    for (uint32_t p0 : act) {
      uint32_t key = 0;
      for (size_t i = 0; i < fixed.size(); ++i) key |= ((p0 >> fixed[i]) & 1u) << i;
      key |= ((p0 >> extra) & 1u) << fixed.size();
      seen |= 1u << key;
    }
    return __builtin_popcount(seen);
  };
  while ((int)fixed.size() < F) {
    int best = -1, best_cnt = 1 << 30;
    for (int b = n - 1; b >= 0; --b) {
      if (b == sel || std::find(fixed.begin(), fixed.end(), b) != fixed.end()) continue;
      const int c = count(b);
      if (c < best_cnt) { best_cnt = c; best = b; }
    }
    if (best < 0 || best_cnt >= 2 * patterns) break;
    fixed.push_back(best);
    patterns = best_cnt;
  }
  return patterns;
}

// LDS bank swizzle of the register path (HamLayout::swz).  ds_read_b128 serves a wavefront in four groups of 16 lanes -
// (lane bit 5, parity of lane bits 2..4) - and a group is conflict free when its 16 lanes hit 16 different 16-byte
// slots modulo 256 B, i.e. 16 different values of index bits 0..3.  The lanes of a unit differ in its free index bits;
// where a low index bit is a hole of the unit (a fixed or the selector bit) the plain layout stacks a group 2, 4 or 8
// deep.  S XORs bits 0..3 with a linear code of bits 4..7: codes c[k] for bit 4+k, coordinate descent from the
// identity and from the best fixed code of all four-hole patterns of 12 bits, scored by the sum over units, waves and
// lane groups of the deepest stack of one slot.  `addr`: the units' member addresses (canonical index << 4) in the
// [trip][thread][unit of the trip] layout.  Returns the swz table and the scores (mean and worst slot depth, 1 =
// conflict free) of the identity and of the chosen map.
struct SwzChoice { uint64_t swz; double mean0, worst0, mean, worst; };
inline SwzChoice choose_bank_swizzle(int lt, const std::vector<uint32_t>& urec, const std::vector<uint32_t>& addr) {
  const size_t NT = (size_t)1 << lt, nu = urec.size();
  std::vector<uint8_t> lo, hi;          // per scored (unit, thread): index bits 0..3 and 4..7
  size_t n_scored = 0;
  for (size_t u = 0; u < nu; ++u) {
    if (!urec[u]) continue;             // zero-table padding
    ++n_scored;
    for (size_t t = 0; t < NT; ++t) {
      const uint32_t p = addr[((u / kUnitTrip) * NT + t) * kUnitTrip + u % kUnitTrip] >> 4;
      lo.push_back((uint8_t)(p & 15u));
      hi.push_back((uint8_t)((p >> 4) & 15u));
    }
  }
  uint8_t grp[4][16];                   // lanes of the four ds_read_b128 groups
  for (int g = 0, cnt[4] = {0, 0, 0, 0}; g < 64; ++g) {
    const int k = ((g >> 5) << 1) | (((g >> 2) ^ (g >> 3) ^ (g >> 4)) & 1);
    grp[k][cnt[k]++] = (uint8_t)g;
  }
  auto table = [](const uint32_t (&c)[4]) {
    uint64_t t = 0;
    for (uint32_t v = 0; v < 16; ++v) {
      uint32_t code = 0;
      for (int k = 0; k < 4; ++k) if ((v >> k) & 1u) code ^= c[k];
      t |= (uint64_t)code << (4 * v);
    }
    return t;
  };
  auto score = [&](uint64_t swz, double* worst) {
    size_t tot = 0;
    int w = 1;
    for (size_t i = 0; i < n_scored * NT; i += 64)
      for (int k = 0; k < 4; ++k) {
        int seen[16] = {0}, m = 0;
        for (int l = 0; l < 16; ++l) {
          const size_t j = i + grp[k][l];
          const int s = lo[j] ^ (int)((swz >> (4 * hi[j])) & 15u);
          m = std::max(m, ++seen[s]);
        }
        tot += m;
        w = std::max(w, m);
      }
    if (worst) *worst = w;
    return n_scored ? (double)tot / (double)(n_scored * NT / 16) : 1.0;
  };
  SwzChoice r{0, 1.0, 1.0, 1.0, 1.0};
  if (!n_scored || lt < 8) return r;
  r.mean0 = r.mean = score(0, &r.worst0);
  r.worst = r.worst0;
  const uint32_t starts[2][4] = {{0u, 0u, 0u, 0u}, {1u, 15u, 2u, 12u}};
  for (const auto& st : starts) {
    uint32_t c[4] = {st[0], st[1], st[2], st[3]};
    double best = score(table(c), nullptr);
    for (int sweep = 0; sweep < 4; ++sweep) {
      bool moved = false;
      for (int k = 0; k < 4; ++k)
        for (uint32_t v = 0; v < 16; ++v) {
          const uint32_t keep = c[k];
          c[k] = v;
          const double s = score(table(c), nullptr);
          if (s < best) { best = s; moved = true; } else c[k] = keep;
        }
      if (!moved) break;
    }
    if (best < r.mean) { r.mean = best; r.swz = table(c); }
  }
  if (r.swz) score(r.swz, &r.worst);
  return r;
}

// ---- the layout: what the energy kernels read (HamDev carries the device copies of these arrays) --------------------
struct HamLayout {
  // group list, X-mask groups of this shard that are not units.  LDS path (n <= 13) order: [diagonal (x == 0) group]
  // [class groups] [plain real groups] [groups that also need an imaginary table]; the class and the plain section
  // are each padded with zero-table dummy groups to a multiple of energy_pd(n).
  std::vector<uint32_t> gx;          // [n_groups] X mask (in the canonical index p', see im)
  std::vector<int32_t> tab_r, tab_i; // [n_groups] offset of the real / imaginary table in `tables` (doubles); tab_i -1: none
  // pair-compacted sign-sum tables D_x(p) = sum_k c_k (-1)^{popc(p & z_k)}, times 2 for x != 0 (the p <-> p^x
  // symmetry).  Entry q of a plain group belongs to the pair representative insert0(q, top_bit(x')), of a class group
  // (layout [j/2][tid][j&1]) to tid | insert0(j, top_bit(x') - LT) << LT, of the diagonal group to index q.
  std::vector<double> tables;
  int has_diag = 0;                  // 1: group 0 is the diagonal group
  int n_real = 0;                    // real-table pair groups incl. zero padding
  // register path (10 <= n <= 13): the state is handed to the energy step in the CANONICAL index p' = M p
  // (GF(2)-linear, chosen so that the X mask of every real group touches one of the R register bits LT..n-1 of p');
  // all masks, tables and addresses of the layout are expressed in p'.  Below the register path M is the identity.
  IndexMap im;
  int n_cls = 0;                     // leading real groups whose x' has a register bit ("class groups", register path only)
  uint32_t mrow[16] = {0};           // row i of S M: bit i of the LDS slot of p' = parity(mrow[i] & p) (the final scatter's map)
  // LDS bank swizzle of the register path (storage only): canonical index p' lives at LDS slot S(p') = p' ^ code(p'),
  // code = 4-bit entry (p' >> 4) & 15 of swz (entry v at bits [4v, 4v+4)); GF(2)-linear, 0 = identity.  Chosen
  // against the unit list's ds_read_b128 lane groups only when the register path has units and every other group
  // is a class group or the diagonal; thread <-> pair ownership does not change.
  uint64_t swz = 0;
  double mean0 = 1.0, worst0 = 1.0, mean = 1.0, worst = 1.0;   // mean / worst slot depth of the unit reads: identity, chosen
  // unit path (8 <= n <= 13): X-mask groups whose sign-sum table is mostly EXACT zeros are stored as *units* -
  // sub-cubes of NT pairs on which the table does not vanish - and never enter the group list.  A unit fixes
  // F = n-1-LT bit positions (plus the selector bit that tells the two members of a pair apart); thread t owns the
  // pair whose remaining LT index bits are the bits of t.  urec: one word per unit, S(x') << 4 (the byte-address
  // distance of the pair members); uaddr: the LDS byte address S(p0) << 4 of the selector-0 member of each
  // (unit, thread); utab: the table values (exactly 0.0 below the zero bound).  uaddr and utab are laid out per trip
  // of kUnitTrip units as [trip][thread][unit of the trip].  The unit count is a multiple of kUnitUnroll (padding:
  // urec 0, tables of zeros, addresses 0).  What is uploaded is unit_arrays() below: these plus the look-ahead trips.
  std::vector<uint32_t> urec, uaddr;
  std::vector<double> utab;
  // explicit terms of the group list (all the streaming path, n >= 14, reads)
  std::vector<int32_t> term_off{0};  // [n_groups + 1]
  std::vector<uint32_t> term_z;      // [n_terms] z' = M^-T z
  std::vector<double> term_cr, term_ci;   // [n_terms] c_k i^{#Y}
};

namespace layout_detail {

constexpr const char* kTooLarge = "Hamiltonian too large for the LDS-resident path";

// Unit path, pass 1, in the qubit order as given: which real groups are sparse, which qubits are their fixed /
// selector bits (hole_freq), the masks of the others (dense_xs).
inline bool classify_sparse_groups(const HamHost& H, int n, int unit_F, const std::vector<int>& mine,
                                   std::vector<char>& sparse, std::vector<uint32_t>& dense_xs, std::vector<int>& hole_freq) {
  const IndexMap id = identity_map(n);
  bool any_sparse = false;
  std::vector<double> D;
  std::vector<uint32_t> act;
  std::vector<int> fixed;
  for (int g : mine) {
    const uint32_t x = H.gx_all[g];
    if (!x || H.group_has_im(g)) continue;
    const int sel = top_bit(x);
    double scale;
    pair_table(H, g, id, n, sel, D, &scale, act);
    const int patterns = choose_fixed_bits(n, sel, unit_F, act, fixed);
    const int units = patterns << (unit_F - (int)fixed.size());
    // a unit costs 2 LDS reads, a group of the class path 2^(F+1) / 2: sparse when no more than half of its
    // sub-cubes are active
    if (2 * units <= (1 << unit_F)) {
      sparse[g] = 1;
      any_sparse = true;
      for (int b : fixed) ++hole_freq[b];
      ++hole_freq[sel];
    } else {
      dense_xs.push_back(x);
    }
  }
  return any_sparse;
}

// Unit path, pass 2, in the canonical index space: the units themselves (urec, uaddr, utab; not yet swizzled)
inline bool build_units(const HamHost& H, int n, int lt, const std::vector<int>& mine, const std::vector<char>& sparse,
                        HamLayout& L, std::string& err) {
  const int unit_F = n - 1 - lt;
  const size_t NT = (size_t)1 << lt;
  std::vector<double> D;
  std::vector<uint32_t> act;
  std::vector<int> fixed;
  for (int g : mine) {
    if (!sparse[g]) continue;
    const uint32_t x = L.im.map_x(H.gx_all[g]);
    const int sel = top_bit(x);
    double scale;
    pair_table(H, g, L.im, n, sel, D, &scale, act);
    choose_fixed_bits(n, sel, unit_F, act, fixed);
    // filler bits: the highest positions that are neither fixed nor the selector
    for (int b = n - 1; b >= 0 && (int)fixed.size() < unit_F; --b)
      if (b != sel && std::find(fixed.begin(), fixed.end(), b) == fixed.end()) fixed.push_back(b);
    uint32_t fmask = 0;
    for (int b : fixed) fmask |= 1u << b;
    std::vector<uint32_t> keys;       // distinct patterns of the fixed bits among the active pairs, ascending
    for (uint32_t p0 : act) keys.push_back(p0 & fmask);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    for (uint32_t s : keys) {
      L.urec.push_back(x << 4);
      for (size_t t = 0; t < NT; ++t) {
        uint32_t p0 = s, tb = 0;       // deposit the bits of t into the free positions, ascending
        for (int b = 0; b < n; ++b)
          if (!((fmask >> b) & 1u) && b != sel) { p0 |= (uint32_t)((t >> tb) & 1u) << b; ++tb; }
        const size_t q = ((size_t)(p0 >> (sel + 1)) << sel) | (p0 & (((size_t)1 << sel) - 1));
        const double d = D[q];
        L.utab.push_back(std::fabs(d) > kUnitZeroTol * scale ? d : 0.0);
        L.uaddr.push_back(p0 << 4);      // LDS byte address of the selector-0 member (the state is 16 bytes per index)
      }
    }
  }
  // (byte offsets into the table array are 31-bit scalars; the padding below and the look-ahead trips of unit_arrays count)
  if (L.utab.size() * sizeof(double) + (size_t)(kUnitUnroll + kUnitAhead) * NT * sizeof(double) > 0x7FFFFFFFu) { err = kTooLarge; return false; }
  // padding to a multiple of kUnitUnroll: units with a table of zeros (both members at address 0)
  while (L.urec.size() % kUnitUnroll) {
    L.urec.push_back(0u);
    L.utab.resize(L.utab.size() + NT, 0.0);
    L.uaddr.resize(L.uaddr.size() + NT, 0u);
  }
  // layout the unit loop reads: per trip of kUnitTrip units [thread][unit of the trip] - a thread's table values of a
  // trip are 32 contiguous bytes, its addresses 16 (one 16-byte load per 2 table values / 4 addresses instead of one
  // 8-byte load per unit, one offset computation per trip: 335.7 -> 331.2 ms on one box)
  auto by_trip = [&](auto& v) {
    std::remove_reference_t<decltype(v)> t(v.size());
    const size_t n_trips = L.urec.size() / kUnitTrip;
    for (size_t T = 0; T < n_trips; ++T)
      for (size_t j = 0; j < (size_t)kUnitTrip; ++j)
        for (size_t th = 0; th < NT; ++th)
          t[(T * NT + th) * kUnitTrip + j] = v[(T * kUnitTrip + j) * NT + th];
    v.swap(t);
  };
  by_trip(L.utab);
  by_trip(L.uaddr);
  return true;
}

// The group list: section order, zero padding, explicit terms and (LDS path) the sign-sum tables
inline bool build_group_list(const HamHost& H, int n, bool lds_path, bool reg_path, int lt, std::vector<int> mine,
                             const std::vector<char>& sparse, HamLayout& L, std::string& err) {
  const size_t dim = (size_t)1 << n;
  const IndexMap& im = L.im;
  auto gxm = [&](int g) { return im.map_x(H.gx_all[g]); };
  // section of a group: 0 diagonal, 1 real with a register bit in x' (register path only),
  // 2 other real groups, 3 groups that also need an imaginary table
  auto rank_of = [&](int g) {
    if (H.group_has_im(g)) return 3;
    const uint32_t x = gxm(g);
    if (x == 0) return 0;
    return reg_path && (x >> lt) ? 1 : 2;
  };
  // ... and inside a section by the top bit of x'
  if (lds_path)
    std::stable_sort(mine.begin(), mine.end(), [&](int a, int b) {
      return rank_of(a) != rank_of(b) ? rank_of(a) < rank_of(b) : top_bit(gxm(a)) > top_bit(gxm(b));
    });
  auto add_dummy = [&](uint32_t xd) {   // zero table: pads a section to a multiple of energy_pd(n)
    L.gx.push_back(xd);
    L.term_off.push_back((int32_t)L.term_z.size());
    L.tab_r.push_back((int32_t)L.tables.size());
    L.tab_i.push_back(-1);
    L.tables.resize(L.tables.size() + dim / 2, 0.0);
  };
  int cur_rank = 0;
  auto enter_section = [&](int rank) {   // rank 4 = end of the list
    if (lds_path) {
      if (cur_rank <= 1 && rank >= 2) while (L.n_cls % energy_pd(n)) { add_dummy(1u << lt); ++L.n_cls; ++L.n_real; }
      if (cur_rank <= 2 && rank >= 3) while ((L.n_real - L.n_cls) % energy_pd(n)) { add_dummy(1u); ++L.n_real; }
    }
    cur_rank = rank;
  };
  std::vector<uint32_t> pidx;
  for (int g : mine) {
    if (sparse[g]) continue;         // lives in the unit list
    const uint32_t x = gxm(g);
    const bool has_im = H.group_has_im(g);
    const int rank = rank_of(g);
    enter_section(rank);
    L.gx.push_back(x);
    for (int k : H.group_terms[g]) {
      L.term_z.push_back(im.map_z((uint32_t)H.hz[k]));
      L.term_cr.push_back(H.hcr[k]);
      L.term_ci.push_back(H.hci[k]);
    }
    L.term_off.push_back((int32_t)L.term_z.size());
    if (!lds_path) {
      L.tab_r.push_back(0);
      L.tab_i.push_back(has_im ? 0 : -1);
      continue;
    }
    if (rank == 0) L.has_diag = 1; else if (!has_im) ++L.n_real;
    if (rank == 1) ++L.n_cls;
    const size_t len = x == 0 ? dim : dim / 2;
    if (L.tables.size() + 2 * len > 0x7FFFFFFFu) { err = kTooLarge; return false; }
    L.tab_r.push_back((int32_t)L.tables.size());
    L.tables.resize(L.tables.size() + len, 0.0);
    if (has_im) { L.tab_i.push_back((int32_t)L.tables.size()); L.tables.resize(L.tables.size() + len, 0.0); }
    else L.tab_i.push_back(-1);
    double* tr = L.tables.data() + L.tab_r.back();
    double* ti = has_im ? L.tables.data() + L.tab_i.back() : nullptr;
    // index of the pair member that entry q of the table belongs to
    pidx.resize(len);
    for (size_t q = 0; q < len; ++q) {
      if (x == 0) pidx[q] = (uint32_t)q;
      else if (rank == 1) {   // [j/2][tid][j&1] with r = insert0(j, cls), p' = tid | r << lt
        const uint32_t t = (uint32_t)((q >> 1) & (((size_t)1 << lt) - 1));
        const uint32_t j = (uint32_t)(((q >> (lt + 1)) << 1) | (q & 1));
        pidx[q] = t | (insert0(j, top_bit(x) - lt) << lt);
      } else {
        pidx[q] = insert0((uint32_t)q, top_bit(x));
      }
    }
    for (int k : H.group_terms[g]) {
      const uint32_t z = im.map_z((uint32_t)H.hz[k]);
      const double factor = x == 0 ? 1.0 : 2.0;      // pair tables carry the factor 2 of the p <-> p^x symmetry
      add_sign_term(tr, 1, pidx, z, factor, H.hcr[k]);
      if (ti) add_sign_term(ti, 1, pidx, z, factor, H.hci[k]);
    }
  }
  enter_section(4);
  return true;
}

}  // namespace layout_detail

// Plans the layout of shard (rank, world) of H.  units_on: the caller's VQE_UNITS switch.  false + err: the
// Hamiltonian does not fit the LDS-resident path.
inline bool plan_hamiltonian(const HamHost& H, int n, bool lds_path, int rank, int world, bool units_on, HamLayout& L,
                             std::string& err) {
  using namespace layout_detail;
  L = HamLayout{};
  const std::vector<int> mine = shard_groups(H, lds_path, rank, world);
  // register path: canonical index p' = M p (see IndexMap); all masks below are in p'
  const bool reg_path = lds_path && n >= kRegMinQubits;
  const int lt = geo_lt(n);                        // Geo<N>::LT of the register path
  const int unit_F = n - 1 - lt;
  L.im = identity_map(n);
  std::vector<char> sparse(H.gx_all.size(), 0);
  bool any_sparse = false;
  if (lds_path && n >= kUnitMinQubits && units_on && unit_F >= 1) {
    std::vector<int> hole_freq(n, 0);
    std::vector<uint32_t> dense_xs;
    any_sparse = classify_sparse_groups(H, n, unit_F, mine, sparse, dense_xs, hole_freq);
    if (any_sparse && reg_path)      // (below the register path the state stays in logical order)
      L.im = choose_permutation(n, lt, dense_xs, hole_freq);
  }
  if (reg_path && !any_sparse) {
    std::vector<uint32_t> xs;
    for (int g : mine) if (H.gx_all[g] && !H.group_has_im(g)) xs.push_back(H.gx_all[g]);
    L.im = choose_index_map(n, lt, xs);
  }
  if (any_sparse && !build_units(H, n, lt, mine, sparse, L, err)) return false;
  if (!build_group_list(H, n, lds_path, reg_path, lt, mine, sparse, L, err)) return false;
  // bank swizzle of the state's LDS copy: register path, units present, and every other group a class group or the
  // diagonal (the plain table paths read the canonical index; a handle with such groups keeps S = I)
  if (reg_path && !L.urec.empty() && L.gx.size() == (size_t)(L.has_diag + L.n_cls)) {
    const SwzChoice sw = choose_bank_swizzle(lt, L.urec, L.uaddr);
    L.swz = sw.swz; L.mean0 = sw.mean0; L.worst0 = sw.worst0; L.mean = sw.mean; L.worst = sw.worst;
  }
  if (L.swz) {
    for (uint32_t& a : L.uaddr) a = swz_slot(L.swz, a >> 4) << 4;
    for (uint32_t& x : L.urec) x = swz_slot(L.swz, x >> 4) << 4;
  }
  for (int i = 0; i < 16; ++i) {     // S M: the final scatter writes canonical index p' to LDS slot S(p')
    uint32_t row = L.im.row[i];
    for (int k = 0; i < 4 && k < 4; ++k)
      if ((L.swz >> (4 * (1 << k)) >> i) & 1u) row ^= L.im.row[4 + k];
    L.mrow[i] = row;
  }
  return true;
}

// The unit arrays as the unit loop (vqe_device.h: unit_energy) reads them: the n_units units of the layout - whole
// turns of accumulated trips - followed by kUnitAhead zero units (record 0, table values 0.0, addresses 0: valid LDS
// addresses).  The loop requests tables and addresses two trips and the record one trip ahead of the trip it
// accumulates; with these look-ahead trips behind the last accumulated one it steps its offsets by constants and
// clamps nothing.  They are only ever prefetched: the loop bound stays n_units.  A layout without units has none.
struct UnitArrays {
  int n_units = 0;                   // accumulated units (HamLayout::urec.size()): the loop bound
  std::vector<uint32_t> urec, uaddr; // [n_units + kUnitAhead], [(n_units + kUnitAhead) * NT]
  std::vector<double> utab;          // [(n_units + kUnitAhead) * NT]
};
inline UnitArrays unit_arrays(const HamLayout& L, int lt) {
  UnitArrays A;
  A.n_units = (int)L.urec.size();
  if (!A.n_units) return A;
  const size_t NT = (size_t)1 << lt, total = L.urec.size() + (size_t)kUnitAhead;
  A.urec = L.urec;   A.urec.resize(total, 0u);
  A.uaddr = L.uaddr; A.uaddr.resize(total * NT, 0u);     // ([trip][thread][unit of the trip]: whole trips go at the end)
  A.utab = L.utab;   A.utab.resize(total * NT, 0.0);
  return A;
}

// ---- adjoint gradient (vqe_grad.h) -----------------------------------------------------------
// The unit-free table set of k_lds_energy_grad: every X-mask group of the shard (the same partition as
// plan_hamiltonian) in the logical index, T[q] = D_x(p0) = sum_k c_k i^{#Y} (-1)^{popc(p0 & z_k)} over the pair
// representatives p0 = insert0(q, top_bit(x)) (complex entries, interleaved, only for groups with an odd number of Y
// factors), the diagonal group over all indices.
struct GradTables {
  std::vector<uint32_t> gx;      // [n_groups] X mask
  std::vector<int64_t> off;      // [n_groups] offset of the group's table in `tab` (doubles)
  std::vector<int32_t> cplx;     // [n_groups] 1: (re, im) entries
  std::vector<double> tab;
};

inline void plan_grad_tables(const HamHost& H, int n, bool lds_path, int rank, int world, GradTables& T) {
  T = GradTables{};
  const size_t dim = (size_t)1 << n;
  std::vector<uint32_t> rep;
  for (int g : shard_groups(H, lds_path, rank, world)) {
    const uint32_t x = H.gx_all[g];
    const bool im = H.group_has_im(g);
    rep.resize(x == 0 ? dim : dim / 2);
    for (size_t q = 0; q < rep.size(); ++q) rep[q] = x == 0 ? (uint32_t)q : insert0((uint32_t)q, top_bit(x));
    T.gx.push_back(x);
    T.off.push_back((int64_t)T.tab.size());
    T.cplx.push_back(im ? 1 : 0);
    const size_t base = T.tab.size();
    T.tab.resize(base + (im ? 2 : 1) * rep.size(), 0.0);
    double* t = T.tab.data() + base;
    for (int k : H.group_terms[g]) {
      add_sign_term(t, im ? 2 : 1, rep, (uint32_t)H.hz[k], 1.0, H.hcr[k]);
      if (im) add_sign_term(t + 1, 2, rep, (uint32_t)H.hz[k], 1.0, H.hci[k]);
    }
  }
}

}  // namespace vqe
