// qj_host_check.cpp - host check of csrc/vqe_qjump.h (tests/test_kraus_traj_cpu.py builds it with g++ and
// -fsanitize=address,undefined and runs it as a program): the channel tables and the compile walk.
//  tables   p_k = sum_j w[k][j] r[j] over the reduced reals against tr(K_k^+ K_k rho_red) from the definition, and
//           sum_k p_k = 1, for amplitude damping, a product set, a non-product set and both depolarising sets; <= 1e-14
//  depol    qj_depol_kraus against sqrt(p / 3) P resp. sqrt(p / 15) P_b (x) P_a at k = a + 4 b; exact
//  quads    qj_quad_bits: the indices with both bits clear meet every coset of span{xm[a], xm[b]} once
//  walk     the records of qj_compile executed naively on a host vector in the frame - rotations by the formulas of the
//           kernel, a jump as a local operator on {p, p ^ xm[a] (, p ^ xm[b], p ^ xm[a] ^ xm[b])} with the local index read
//           off the parities - against a physical-frame simulation of the same gate list with the same operator choice
//           (k = g mod count, then normalised); random circuits with CNOT chains, all six rotation kinds and both slot
//           kinds at n = 2, 3, 5; max |amplitude difference| <= 1e-13.  The reduced reals of every jump agree as well.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "vqe_qjump.h"

using namespace vqe;
typedef std::complex<double> cd;

static int fails = 0;
static void check(bool ok, const char* what, double v) {
  if (!ok) { std::printf("FAIL %s %.3e\n", what, v); ++fails; }
}
static int par(uint32_t v) { return __builtin_popcount(v) & 1; }

static std::vector<cd> amp_damp(double g) { return {1.0, 0.0, 0.0, std::sqrt(1.0 - g), 0.0, std::sqrt(g), 0.0, 0.0}; }
static std::vector<cd> dephase(double p) { return {std::sqrt(1.0 - p), 0.0, 0.0, std::sqrt(1.0 - p), std::sqrt(p), 0.0, 0.0, -std::sqrt(p)}; }
// Ka on q0 (low index bit), Kb on q1
static std::vector<cd> tensor(const std::vector<cd>& Ka, const std::vector<cd>& Kb) {
  std::vector<cd> K;
  for (size_t a = 0; a < Ka.size() / 4; ++a) for (size_t b = 0; b < Kb.size() / 4; ++b)
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c)
      K.push_back(Ka[a * 4 + (r & 1) * 2 + (c & 1)] * Kb[b * 4 + (r >> 1) * 2 + (c >> 1)]);
  return K;
}
static std::vector<cd> cnot_mix() {      // {sqrt 0.7 1, sqrt 0.3 CNOT(q0 -> q1)}: index = bit(q0) + 2 bit(q1)
  std::vector<cd> K(32, 0.0);
  for (int i = 0; i < 4; ++i) K[i * 4 + i] = std::sqrt(0.7);
  const int perm[4] = {0, 3, 2, 1};
  for (int i = 0; i < 4; ++i) K[16 + perm[i] * 4 + i] = std::sqrt(0.3);
  return K;
}

// the reduced reals of local amplitudes a[group][d], in the order of qj_build_tables
static std::vector<double> reduced_reals(const std::vector<std::vector<cd>>& groups, int d) {
  std::vector<double> r(d * d, 0.0);
  for (const auto& a : groups) {
    for (int i = 0; i < d; ++i) r[i] += std::norm(a[i]);
    int t = d;
    for (int i = 0; i < d; ++i) for (int j = i + 1; j < d; ++j) {
      const cd rho_ji = a[j] * std::conj(a[i]);
      r[t++] += rho_ji.real();
      r[t++] += rho_ji.imag();
    }
  }
  return r;
}

static double check_tables(const std::vector<cd>& K, int d, std::mt19937_64& rng) {
  const int count = (int)K.size() / (d * d);
  std::vector<double> k, w;
  qj_build_tables(K.data(), count, d, k, w);
  std::normal_distribution<double> N(0.0, 1.0);
  double worst = 0.0;
  for (int rep = 0; rep < 20; ++rep) {
    std::vector<std::vector<cd>> groups(3, std::vector<cd>(d));
    double nrm = 0.0;
    for (auto& g : groups) for (auto& a : g) { a = cd(N(rng), N(rng)); nrm += std::norm(a); }
    for (auto& g : groups) for (auto& a : g) a /= std::sqrt(nrm);
    const std::vector<double> r = reduced_reals(groups, d);
    double sum = 0.0;
    for (int kk = 0; kk < count; ++kk) {
      double p = 0.0, ref = 0.0;
      for (int j = 0; j < d * d; ++j) p += w[kk * d * d + j] * r[j];
      for (const auto& g : groups) for (int i = 0; i < d; ++i) {      // |K a|^2 summed over the groups
        cd v = 0.0;
        for (int j = 0; j < d; ++j) v += K[(kk * d + i) * d + j] * g[j];
        ref += std::norm(v);
      }
      worst = std::max(worst, std::abs(p - ref));
      sum += p;
    }
    worst = std::max(worst, std::abs(sum - 1.0));
  }
  for (size_t e = 0; e < K.size(); ++e) worst = std::max(worst, std::abs(cd(k[2 * e], k[2 * e + 1]) - K[e]));
  return worst;
}

struct Gate { int kind, q0, q1, pidx; };

static cd pauli(int p, int r, int c) {
  static const cd P[4][4] = {{1.0, 0.0, 0.0, 1.0}, {0.0, 1.0, 1.0, 0.0}, {0.0, cd(0.0, -1.0), cd(0.0, 1.0), 0.0}, {1.0, 0.0, 0.0, -1.0}};
  return P[p][r * 2 + c];
}

// physical frame: a d x d operator on qubits (qa[, qb]), local index = bit(qa) + 2 bit(qb)
static void apply_phys(std::vector<cd>& v, int n, int qa, int qb, const cd* m, int d, std::vector<double>* reals) {
  std::vector<std::vector<cd>> groups;
  std::vector<std::vector<uint32_t>> idx;
  for (uint32_t i = 0; i < (1u << n); ++i) {
    if (((i >> qa) & 1u) || (d == 4 && ((i >> qb) & 1u))) continue;
    std::vector<uint32_t> mem(d);
    std::vector<cd> a(d);
    for (int l = 0; l < d; ++l) { mem[l] = i | ((uint32_t)(l & 1) << qa) | (d == 4 ? (uint32_t)(l >> 1) << qb : 0u); a[l] = v[mem[l]]; }
    groups.push_back(a);
    idx.push_back(mem);
  }
  if (reals) *reals = reduced_reals(groups, d);
  for (size_t g = 0; g < groups.size(); ++g)
    for (int i = 0; i < d; ++i) {
      cd s = 0.0;
      for (int j = 0; j < d; ++j) s += m[i * d + j] * groups[g][j];
      v[idx[g][i]] = s;
    }
}
static void normalise(std::vector<cd>& v) {
  double s = 0.0;
  for (const cd& a : v) s += std::norm(a);
  for (cd& a : v) a /= std::sqrt(s);
}

static double check_walk(int n, int G, bool slot1, bool slot2, uint64_t seed, double* worst_reals) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(-3.14159, 3.14159);
  std::normal_distribution<double> N(0.0, 1.0);
  const std::vector<cd> K1 = amp_damp(0.3), K2 = tensor(amp_damp(0.25), dephase(0.2));
  const std::vector<cd> K2b = cnot_mix();
  const bool use_b = (seed & 1) != 0;
  const std::vector<cd>& KK2 = use_b ? K2b : K2;
  const int n1 = 2, n2 = (int)KK2.size() / 16;
  std::vector<GateRec> g;
  std::vector<double> theta;
  const int rot_kinds[6] = {G_RX, G_RY, G_RZ, G_RXX, G_RYY, G_RZZ};
  for (int i = 0; i < G; ++i) {
    const int a = (int)(rng() % n), b = (int)((a + 1 + rng() % (n - 1)) % n);
    const int what = (int)(rng() % 10);
    if (what < 3) {                                    // a CNOT chain of 1 .. 3
      int c = a;
      for (int l = 0, len = 1 + (int)(rng() % 3); l < len; ++l) {
        const int t = (int)((c + 1 + rng() % (n - 1)) % n);
        g.push_back(GateRec{G_CNOT, c, t, -1});
        g.push_back(GateRec{G_DEPOL2, c, t, -1});
        c = t;
      }
    } else {
      const int k = rot_kinds[rng() % 6];
      g.push_back(GateRec{k, a, gate_is_rot2(k) ? b : -1, (int)theta.size()});
      theta.push_back(U(rng));
      g.push_back(gate_is_rot2(k) ? GateRec{G_DEPOL2, b, a, -1} : GateRec{G_DEPOL1, a, -1, -1});      // (q0, q1 in the other order)
    }
  }
  std::vector<cd> phys(1u << n);
  for (cd& a : phys) a = cd(N(rng), N(rng));
  normalise(phys);
  std::vector<cd> frame = phys;      // the walk starts at the identity map: the frame is the physical one

  // ---- the frame run
  std::vector<QjOp> ops(4 * g.size() + 4);
  uint32_t xm[32], zm[32], c = 0;
  const int need = qj_compile(g.data(), (int)g.size(), n, slot1, slot2, ops.data(), (int)ops.size(), xm, zm, &c);
  if (need > (int)ops.size()) { check(false, "record count", need); return 1.0; }
  {      // capacity: a walk into a short buffer writes nothing beyond it (the sanitizer watches) and counts the same
    std::vector<QjOp> few(need / 2);
    uint32_t x2[32], z2[32], c2;
    check(qj_compile(g.data(), (int)g.size(), n, slot1, slot2, few.data(), (int)few.size(), x2, z2, &c2) == need, "short buffer count", 0);
  }
  for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) check(par(zm[a] & xm[b]) == (a == b), "zm . xm = delta", a * 32 + b);
  std::vector<std::vector<double>> frame_reals, phys_reals;
  for (int o = 0; o < need; ++o) {
    const QjOp op = ops[o];
    const int kind = op.kind & 0xff, inv = (op.kind >> 8) & 1;
    if (kind == G_RX || kind == G_RY || kind == G_RYY || kind == G_RZ) {
      const double cs = std::cos(0.5 * theta[op.arg]), sn = std::sin(0.5 * theta[op.arg]);
      if (kind == G_RZ) {
        for (uint32_t p = 0; p < (1u << n); ++p) frame[p] *= cd(cs, (par(p & op.zm) ^ inv) ? -sn : sn);
        continue;
      }
      int hb = 0;
      for (int q = 0; q < 32; ++q) if ((op.xm >> q) & 1u) hb = q;
      for (uint32_t p0 = 0; p0 < (1u << n); ++p0) {
        if ((p0 >> hb) & 1u) continue;
        const uint32_t p1 = p0 ^ op.xm;
        const cd a0 = frame[p0], a1 = frame[p1];
        if (kind == G_RX) {
          frame[p0] = cs * a0 + cd(0.0, sn) * a1;
          frame[p1] = cs * a1 + cd(0.0, sn) * a0;
        } else if (kind == G_RY) {
          const double s0 = (par(p0 & op.zm) ^ inv) ? -sn : sn;
          frame[p0] = cs * a0 + s0 * a1;
          frame[p1] = cs * a1 - s0 * a0;
        } else {
          const double s0 = (par(p0 & op.zm) ^ inv) ? sn : -sn;
          frame[p0] = cs * a0 + cd(0.0, s0) * a1;
          frame[p1] = cs * a1 + cd(0.0, s0) * a0;
        }
      }
    } else if (kind == QJ_JUMP1 || kind == QJ_JUMP2) {
      const int d = kind == QJ_JUMP1 ? 2 : 4;
      const QjOp ob = d == 4 ? ops[o + 1] : QjOp{0u, 0u, 0, 0};
      const int invb = (op.kind >> 9) & 1;
      if (d == 4) { check((ob.kind & 0xff) == QJ_TAIL, "tail record", o); ++o; }
      const cd* K = (d == 2 ? K1.data() : KK2.data()) + (size_t)(op.arg % (d == 2 ? n1 : n2)) * d * d;
      if (d == 4) {
        int lo, hi, reps = 0;
        qj_quad_bits(op.xm, ob.xm, &lo, &hi);
        std::vector<int> seen(1u << n, 0);
        for (uint32_t p = 0; p < (1u << n); ++p) {
          if (((p >> lo) & 1u) || ((p >> hi) & 1u)) continue;
          ++reps;
          for (int s = 0; s < 4; ++s) ++seen[p ^ ((s & 1) ? op.xm : 0u) ^ ((s & 2) ? ob.xm : 0u)];
        }
        bool once = reps == (1 << n) / 4 && lo < hi;
        for (int v : seen) once = once && v == 1;
        check(once, "quad representatives", o);
      }
      std::vector<std::vector<cd>> groups;
      std::vector<std::vector<uint32_t>> idx;
      for (uint32_t p = 0; p < (1u << n); ++p) {
        if ((par(p & op.zm) ^ inv) || (d == 4 && (par(p & ob.zm) ^ invb))) continue;      // local index 0
        std::vector<uint32_t> mem(d);
        std::vector<cd> a(d);
        for (int l = 0; l < d; ++l) { mem[l] = p ^ ((l & 1) ? op.xm : 0u) ^ ((l & 2) ? ob.xm : 0u); a[l] = frame[mem[l]]; }
        groups.push_back(a);
        idx.push_back(mem);
      }
      frame_reals.push_back(reduced_reals(groups, d));
      for (size_t gi = 0; gi < groups.size(); ++gi)
        for (int i = 0; i < d; ++i) {
          cd s = 0.0;
          for (int j = 0; j < d; ++j) s += K[i * d + j] * groups[gi][j];
          frame[idx[gi][i]] = s;
        }
      normalise(frame);
    } else {
      check(false, "unknown record", kind);
    }
  }
  // ---- the physical run
  for (size_t i = 0; i < g.size(); ++i) {
    const GateRec r = g[i];
    if (r.kind == G_CNOT) {
      const cd cx[16] = {1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0};
      apply_phys(phys, n, r.q0, r.q1, cx, 4, nullptr);
    } else if (r.kind >= G_RX && r.kind <= G_RZ) {
      const double t = theta[r.pidx];
      cd m[4];
      for (int e = 0; e < 4; ++e) m[e] = std::cos(t / 2) * pauli(0, e >> 1, e & 1) + cd(0.0, std::sin(t / 2)) * pauli(r.kind, e >> 1, e & 1);
      apply_phys(phys, n, r.q0, -1, m, 2, nullptr);
    } else if (gate_is_rot2(r.kind)) {
      const double t = theta[r.pidx];
      const int p = r.kind - G_RXX + 1;
      cd m[16];
      for (int rr = 0; rr < 4; ++rr) for (int cc = 0; cc < 4; ++cc)
        m[rr * 4 + cc] = std::cos(t / 2) * (rr == cc ? 1.0 : 0.0) + cd(0.0, std::sin(t / 2)) * pauli(p, rr & 1, cc & 1) * pauli(p, rr >> 1, cc >> 1);
      apply_phys(phys, n, r.q0, r.q1, m, 4, nullptr);
    } else if ((r.kind == G_DEPOL1 && slot1) || (r.kind == G_DEPOL2 && slot2)) {
      const int d = r.kind == G_DEPOL1 ? 2 : 4;
      const cd* K = (d == 2 ? K1.data() : KK2.data()) + (size_t)((int)i % (d == 2 ? n1 : n2)) * d * d;
      std::vector<double> reals;
      apply_phys(phys, n, r.q0, r.q1, K, d, &reals);
      phys_reals.push_back(reals);
      normalise(phys);
    }
  }
  double worst = 0.0;
  for (uint32_t p = 0; p < (1u << n); ++p) {
    uint32_t i = 0;
    for (int a = 0; a < n; ++a) i |= (uint32_t)(par(p & zm[a]) ^ ((c >> a) & 1u)) << a;
    worst = std::max(worst, std::abs(frame[p] - phys[i]));
  }
  check(frame_reals.size() == phys_reals.size(), "jump count", (double)frame_reals.size());
  for (size_t j = 0; j < frame_reals.size() && j < phys_reals.size(); ++j)
    for (size_t e = 0; e < frame_reals[j].size(); ++e) *worst_reals = std::max(*worst_reals, std::abs(frame_reals[j][e] - phys_reals[j][e]));
  return worst;
}

int main() {
  std::mt19937_64 rng(2024);
  double wt = 0.0;
  wt = std::max(wt, check_tables(amp_damp(0.3), 2, rng));
  wt = std::max(wt, check_tables(dephase(0.2), 2, rng));
  wt = std::max(wt, check_tables(tensor(amp_damp(0.25), dephase(0.2)), 4, rng));
  wt = std::max(wt, check_tables(cnot_mix(), 4, rng));
  std::vector<cd> d1, d2;
  qj_depol_kraus(0.2, 2, d1);
  qj_depol_kraus(0.4, 4, d2);
  wt = std::max(wt, check_tables(d1, 2, rng));
  wt = std::max(wt, check_tables(d2, 4, rng));
  check(wt <= 1e-14, "tables", wt);
  std::printf("tables %.3e\n", wt);
  double wd = 0.0;
  check(d1.size() == 16 && d2.size() == 256, "depol sizes", (double)d2.size());
  for (int a = 0; a < 4; ++a) for (int e = 0; e < 4; ++e)
    wd = std::max(wd, std::abs(d1[a * 4 + e] - std::sqrt(a ? 0.2 / 3.0 : 0.8) * pauli(a, e >> 1, e & 1)));
  for (int k = 0; k < 16; ++k) for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c)
    wd = std::max(wd, std::abs(d2[k * 16 + r * 4 + c] - std::sqrt(k ? 0.4 / 15.0 : 0.6) * pauli(k & 3, r & 1, c & 1) * pauli(k >> 2, r >> 1, c >> 1)));
  check(wd == 0.0, "depol", wd);
  std::printf("depol %.3e\n", wd);
  double ww = 0.0, wr = 0.0;
  int cases = 0;
  for (int n : {2, 3, 5})
    for (uint64_t s = 0; s < 12; ++s) {
      const bool s1 = s % 6 != 4, s2 = s % 6 != 5;      // also: one slot the identity
      ww = std::max(ww, check_walk(n, 14, s1, s2, 100 * n + s, &wr));
      ++cases;
    }
  check(ww <= 1e-13, "walk", ww);
  check(wr <= 1e-13, "walk reduced reals", wr);
  std::printf("walk %.3e reals %.3e cases %d\n", ww, wr, cases);
  std::printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
