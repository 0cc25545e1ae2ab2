// dm_channel_check.cpp - CPU check of the Kraus channel tables and the two-qubit rotation members of the exact channel
// mode (csrc/dm_host.h, csrc/dm_build.h).  Host only; built by tests/test_dm_channels_cpu.py with g++.
//
//   (a) sup_kraus_1q / sup_kraus_2q of the depolarising Kraus sets equal sup_depol, <= 1e-15 per entry, on both window
//       positions and in both orientations; dm_channel_tables lays them out as the four slices;
//   (b) the swapped two-qubit table equals the table of the qubit-exchanged Kraus set (same bits), and for
//       amplitude damping (x) identity the damped qubit is the gate's q0 in both orientations;
//   (c) dm_member_entry for RXX / RYY / RZZ equals the superoperator dm_fill_blocks builds for that member, and the
//       dm_build_entry chain of whole blocks - rotations, CNOTs, two-qubit rotations, Kraus channels in both slots -
//       equals the fill, <= 1e-14 per entry;
//   (d) dm_block_derivative through every rotation member, two-qubit ones included, equals the exact shift
//       (S(theta + pi/2) - S(theta - pi/2)) / 2 of the filled block, <= 1e-13 relative to the largest entry;
//   (e) without an override and without rot2 the plan is member for member the planner's from before this file's
//       features (kept below as plan_before), with DEPOL2.pos == 0; with a two-qubit override only DEPOL2.pos changes,
//       to the window position of the gate's q0.
// Circuits are drawn here from a fixed linear congruential generator; prints "ok" last.
#include "dm_host.h"
#include "dm_build.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

using namespace vqe;

static void CHECK(bool ok, const char* fmt, ...) {
  if (ok) return;
  va_list ap;
  va_start(ap, fmt);
  std::fprintf(stderr, "FAILED: ");
  std::vfprintf(stderr, fmt, ap);
  std::fprintf(stderr, "\n");
  va_end(ap);
  std::exit(1);
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_seed >> 33); }
static double unif() { return (rnd() + 0.5) / 2147483648.0; }      // (0, 1)

static double sup_diff(const Sup& x, const Sup& y) {
  double d = 0.0;
  for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) d = std::max(d, std::abs(x.m[r][c] - y.m[r][c]));
  return d;
}

static std::vector<cplx> depol1_kraus(double p) {
  std::vector<cplx> K;
  for (int k = 0; k < 4; ++k) {
    cplx R[2][2];
    pauli_1q(k, R);
    const double w = std::sqrt(k == 0 ? 1.0 - p : p / 3.0);
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) K.push_back(w * R[i][j]);
  }
  return K;
}
static std::vector<cplx> depol2_kraus(double p) {      // index = bit(q0) + 2 bit(q1)
  std::vector<cplx> K;
  for (int pb = 0; pb < 4; ++pb) for (int pa = 0; pa < 4; ++pa) {
    cplx Ra[2][2], Rb[2][2];
    pauli_1q(pa, Ra); pauli_1q(pb, Rb);
    const double w = std::sqrt((pa || pb) ? p / 15.0 : 1.0 - p);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) K.push_back(w * Ra[i & 1][j & 1] * Rb[i >> 1][j >> 1]);
  }
  return K;
}
// amplitude damping on q0 (x) identity on q1
static std::vector<cplx> damp_q0_kraus(double gamma) {
  const cplx k0[2][2] = {{1.0, 0.0}, {0.0, std::sqrt(1.0 - gamma)}}, k1[2][2] = {{0.0, std::sqrt(gamma)}, {0.0, 0.0}};
  std::vector<cplx> K;
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) K.push_back((i >> 1) == (j >> 1) ? (k ? k1 : k0)[i & 1][j & 1] : cplx(0.0));
  return K;
}
static std::vector<cplx> random_kraus(int count, int d) {      // any operators: the table identities are linear in them
  std::vector<cplx> K((size_t)count * d * d);
  for (cplx& v : K) v = cplx(unif() - 0.5, unif() - 0.5);
  return K;
}

// dm_plan_blocks as it was before Kraus channels and two-qubit rotations
static void plan_before(int n, const GateRec* g, int G, std::vector<DmBlockPlan>& out) {
  out.clear();
  std::vector<DmBlockPlan> open;
  auto owner = [&](int q) { for (size_t k = 0; k < open.size(); ++k) if (open[k].a == q || open[k].b == q) return (int)k; return -1; };
  auto close = [&](int k) { out.push_back(std::move(open[k])); open.erase(open.begin() + k); };
  for (int i = 0; i < G; ++i) {
    const GateRec r = g[i];
    const bool two = r.kind == G_CNOT || r.kind == G_DEPOL2;
    const int qa = r.q0, qb = two ? r.q1 : -1;
    int k = owner(qa);
    const int k2 = two ? owner(qb) : k;
    if (k < 0 || k2 != k) {
      const int c1 = k, c2 = two ? k2 : -1;
      if (c1 >= 0 && c2 >= 0 && c1 != c2) { close(std::max(c1, c2)); close(std::min(c1, c2)); }
      else if (c1 >= 0) close(c1);
      else if (c2 >= 0) close(c2);
      DmBlockPlan nb{};
      nb.a = qa;
      nb.b = qb;
      if (nb.b < 0) {
        int want = -1;
        for (int j = i + 1; j < G && want < 0; ++j) {
          const bool t2 = g[j].kind == G_CNOT || g[j].kind == G_DEPOL2;
          if (t2 && g[j].q0 == qa) want = g[j].q1;
          else if (t2 && g[j].q1 == qa) want = g[j].q0;
        }
        if (want >= 0 && owner(want) < 0) nb.b = want;
        for (int q = 0; q < n && nb.b < 0; ++q) if (q != qa && owner(q) < 0) nb.b = q;
        if (nb.b < 0) { nb.b = open[0].a; close(0); }
      }
      open.push_back(std::move(nb));
      k = (int)open.size() - 1;
    }
    DmBlockPlan& cur = open[k];
    const int pos = r.q0 == cur.a ? 0 : 1;
    cur.members.push_back(DmMember{r.kind, r.kind == G_DEPOL2 ? 0 : pos, (r.kind >= G_RX && r.kind <= G_RZ) ? r.pidx : -1});
  }
  while (!open.empty()) close(0);
}

// a random circuit with a channel behind every gate; rot2: two-qubit rotations among the gates
static void random_circuit(int n, int G, bool rot2, std::vector<GateRec>& g, std::vector<double>& th) {
  g.clear();
  th.clear();
  for (int i = 0; i < G; ++i) {
    const int a = (int)(rnd() % n), b = (a + 1 + (int)(rnd() % (n - 1))) % n, pick = (int)(rnd() % (rot2 ? 3 : 2));
    if (pick == 0) {
      g.push_back(GateRec{G_CNOT, a, b, -1});
      g.push_back(GateRec{G_DEPOL2, (rnd() & 1) ? a : b, -1, -1});
      g.back().q1 = g.back().q0 == a ? b : a;      // the channel in either order of the CNOT's qubits
    } else if (pick == 1) {
      g.push_back(GateRec{G_RX + (int)(rnd() % 3), a, -1, (int)th.size()});
      th.push_back((unif() - 0.5) * 6.0);
      g.push_back(GateRec{G_DEPOL1, a, -1, -1});
    } else {
      g.push_back(GateRec{G_RXX + (int)(rnd() % 3), a, b, (int)th.size()});
      th.push_back((unif() - 0.5) * 6.0);
      g.push_back(GateRec{G_DEPOL2, b, a, -1});
    }
  }
}

// the dm_build_entry chain of one block -> Sup
static void chain(const DmBlockPlan& blk, const double* th, const std::vector<double>& dep, Sup& out) {
  static double s[2][2][256];
  int cur = 0;
  for (int t = 0; t < 256; ++t) { s[0][0][t] = (t >> 4) == (t & 15) ? 1.0 : 0.0; s[0][1][t] = 0.0; }
  for (const DmMember& m : blk.members) {
    const double cs = m.pidx >= 0 ? std::cos(0.5 * th[m.pidx]) : 1.0, sn = m.pidx >= 0 ? std::sin(0.5 * th[m.pidx]) : 0.0;
    for (int t = 0; t < 256; ++t)
      dm_build_entry(m.kind, m.pos, cs, sn, dep.data(), s[cur][0], s[cur][1], t >> 4, t & 15, s[cur ^ 1][0][t], s[cur ^ 1][1][t]);
    cur ^= 1;
  }
  for (int t = 0; t < 256; ++t) out.m[t >> 4][t & 15] = cplx(s[cur][0][t], s[cur][1][t]);
}

int main() {
  const double kHalfPi = 1.57079632679489661923;
  double worst_a = 0.0, worst_c = 0.0, worst_d = 0.0;

  // (a) depolarising Kraus sets against sup_depol
  for (double p : {0.0, 0.01, 0.05, 0.3, 0.75, 1.0}) {
    const std::vector<cplx> K1 = depol1_kraus(p), K2 = depol2_kraus(p);
    CHECK(kraus_tp_defect(K1.data(), 4, 2) <= 1e-15 && kraus_tp_defect(K2.data(), 16, 4) <= 1e-15, "depolarising Kraus sets are trace preserving");
    for (int pos = 0; pos < 2; ++pos) {
      Sup A, B;
      sup_kraus_1q(K1.data(), 4, pos, A);
      sup_depol(pos + 1, p, B);
      worst_a = std::max(worst_a, sup_diff(A, B));
    }
    for (int sw = 0; sw < 2; ++sw) {
      Sup A, B;
      sup_kraus_2q(K2.data(), 16, sw != 0, A);
      sup_depol(3, p, B);
      worst_a = std::max(worst_a, sup_diff(A, B));
    }
    DmKraus kr;
    kr.n1 = 4; kr.K1 = K1; kr.n2 = 16; kr.K2 = K2;
    std::vector<double> four, three;
    dm_channel_tables(0.5, 0.5, &kr, four);
    dm_depol_tables(p, p, three);
    CHECK(four.size() == 4 * 512 && three.size() == 3 * 512, "table sizes");
    for (int w = 0; w < 4; ++w) for (int t = 0; t < 512; ++t) worst_a = std::max(worst_a, std::abs(four[w * 512 + t] - three[std::min(w, 2) * 512 + t]));
  }
  CHECK(worst_a <= 1e-15, "Kraus tables of the depolarising sets differ from sup_depol by %.3e", worst_a);
  {
    const cplx bad[4] = {1.0, 0.0, 0.0, 0.5};
    CHECK(kraus_tp_defect(bad, 1, 2) > 0.7, "a set that loses trace is seen");
    const double nan = std::nan("");
    const cplx none[4] = {nan, nan, nan, nan}, some[4] = {1.0, 0.0, cplx(0.0, nan), 1.0};
    CHECK(!(kraus_tp_defect(none, 1, 2) <= 1e-12) && !(kraus_tp_defect(some, 1, 2) <= 1e-12), "a set with NaN entries is seen");
    std::vector<cplx> near = depol1_kraus(0.3);
    for (int t = 12; t < 16; ++t) near[t] *= 1.0 + 1e-11;      // the Z operator a little too long: defect 2e-12 p/3
    CHECK(kraus_tp_defect(near.data(), 4, 2) > 1e-12 && kraus_tp_defect(near.data(), 4, 2) < 1e-11, "the bound resolves 2e-12");
  }

  // (b) orientation
  for (int trial = 0; trial < 8; ++trial) {
    const int cnt = 1 + (int)(rnd() % 5);
    const std::vector<cplx> K = random_kraus(cnt, 4);
    std::vector<cplx> X(K.size());
    const auto sw = [](int i) { return ((i & 1) << 1) | (i >> 1); };
    for (int k = 0; k < cnt; ++k) for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) X[16 * k + 4 * sw(i) + sw(j)] = K[16 * k + 4 * i + j];
    Sup A, B, C;
    sup_kraus_2q(K.data(), cnt, true, A);
    sup_kraus_2q(X.data(), cnt, false, B);
    sup_kraus_2q(K.data(), cnt, false, C);
    CHECK(sup_diff(A, B) == 0.0, "swapped table differs from the table of the exchanged set");
    CHECK(sup_diff(A, C) > 1e-3, "a random set is not symmetric under exchange");
  }
  {
    const double gamma = 0.3;
    const std::vector<cplx> K = damp_q0_kraus(gamma);
    CHECK(kraus_tp_defect(K.data(), 2, 4) <= 1e-15, "damping (x) identity is trace preserving");
    Sup A, B;
    sup_kraus_2q(K.data(), 2, false, A);      // q0 = window qubit a = bit 0
    sup_kraus_2q(K.data(), 2, true, B);       // q0 = window qubit b = bit 1
    // |11><11| is entry 3 + 4 * 3; the damped qubit falls to 0 with probability gamma
    CHECK(std::abs(A.m[2 + 4 * 2][15] - gamma) <= 1e-15 && std::abs(A.m[15][15] - (1.0 - gamma)) <= 1e-15 && std::abs(A.m[1 + 4 * 1][15]) == 0.0,
          "unswapped: qubit a is the damped one");
    CHECK(std::abs(B.m[1 + 4 * 1][15] - gamma) <= 1e-15 && std::abs(B.m[15][15] - (1.0 - gamma)) <= 1e-15 && std::abs(B.m[2 + 4 * 2][15]) == 0.0,
          "swapped: qubit b is the damped one");
  }

  // (c) two-qubit rotation members, one at a time
  const std::vector<double> no_dep(4 * 512, 0.0);
  for (int kind = G_RXX; kind <= G_RZZ; ++kind) for (int pos = 0; pos < 2; ++pos) for (int trial = 0; trial < 4; ++trial) {
    const double th = (unif() - 0.5) * 6.0;
    std::vector<DmBlockPlan> one(1);
    one[0].a = 0; one[0].b = 1;
    one[0].members.push_back(DmMember{kind, pos, 0});
    std::vector<DmBlockHost> filled;
    dm_fill_blocks(one, &th, 0.0, 0.0, filled);
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
      double gr, gi;
      dm_member_entry(kind, pos, std::cos(0.5 * th), std::sin(0.5 * th), no_dep.data(), r, c, gr, gi);
      CHECK(std::abs(cplx(gr, gi) - filled[0].S.m[r][c]) <= 1e-15, "member entry of kind %d (%d, %d)", kind, r, c);
    }
    // unitary: S S^+ = 1
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
      cplx v = 0.0;
      for (int k = 0; k < 16; ++k) v += filled[0].S.m[r][k] * std::conj(filled[0].S.m[c][k]);
      CHECK(std::abs(v - (r == c ? 1.0 : 0.0)) <= 1e-14, "two-qubit rotation is not unitary");
    }
  }

  // (c), (d) whole blocks with every kind of member; (e) plans
  long n_rot2 = 0, n_swapped = 0, n_blocks = 0, n_deriv = 0;
  for (int n : {2, 3, 5, 8}) for (int trial = 0; trial < 6; ++trial) {
    std::vector<GateRec> g;
    std::vector<double> th;
    DmKraus kr;
    kr.n1 = 2; kr.K1 = {1.0, 0.0, 0.0, std::sqrt(0.75), 0.0, 0.5, 0.0, 0.0};      // amplitude damping, gamma = 1/4
    if (trial & 1) { kr.n2 = 2; kr.K2 = damp_q0_kraus(0.4); }                       // odd trials: both slots, even: one slot
    std::vector<double> dep;
    dm_channel_tables(0.07, 0.11, &kr, dep);
    const DmPlanOpts opt{kr.n2 > 0, true};
    random_circuit(n, 4 + 6 * trial, true, g, th);
    std::vector<DmBlockPlan> plan;
    dm_plan_blocks(n, g.data(), (int)g.size(), plan, opt);
    std::vector<DmBlockHost> filled, up, dn;
    dm_fill_blocks(plan, th.data(), 0.07, 0.11, filled, &kr);
    size_t members = 0;
    for (size_t k = 0; k < plan.size(); ++k) {
      ++n_blocks;
      members += plan[k].members.size();
      Sup C;
      chain(plan[k], th.data(), dep, C);
      worst_c = std::max(worst_c, sup_diff(C, filled[k].S));
      std::vector<int32_t> mem;
      std::vector<double> cs, sn;
      for (const DmMember& m : plan[k].members) {
        mem.insert(mem.end(), {m.kind, m.pos, m.pidx});
        cs.push_back(m.pidx >= 0 ? std::cos(0.5 * th[m.pidx]) : 1.0);
        sn.push_back(m.pidx >= 0 ? std::sin(0.5 * th[m.pidx]) : 0.0);
        if (gate_is_rot2(m.kind)) { ++n_rot2; CHECK(m.pidx >= 0, "a two-qubit rotation keeps its parameter"); }
        if (m.kind == G_DEPOL2 && m.pos == 1) ++n_swapped;
        if (m.kind == G_DEPOL2 && !opt.orient2) CHECK(m.pos == 0, "DEPOL2.pos without a two-qubit override");
      }
      for (size_t w = 0; w < plan[k].members.size(); ++w) {
        const DmMember& d = plan[k].members[w];
        if (d.pidx < 0) continue;
        ++n_deriv;
        static double o[2][256], t[2][256];
        dm_block_derivative(mem.data(), (int)plan[k].members.size(), (int)w, cs.data(), sn.data(), dep.data(), o[0], o[1], t[0], t[1]);
        std::vector<DmBlockPlan> one(1, plan[k]);
        const double keep = th[d.pidx];      // (every parameter belongs to one gate here)
        th[d.pidx] = keep + kHalfPi; dm_fill_blocks(one, th.data(), 0.07, 0.11, up, &kr);
        th[d.pidx] = keep - kHalfPi; dm_fill_blocks(one, th.data(), 0.07, 0.11, dn, &kr);
        th[d.pidx] = keep;
        double big = 1.0;
        for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) big = std::max(big, std::abs(0.5 * (up[0].S.m[r][c] - dn[0].S.m[r][c])));
        for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c)
          worst_d = std::max(worst_d, std::abs(cplx(o[0][r * 16 + c], o[1][r * 16 + c]) - 0.5 * (up[0].S.m[r][c] - dn[0].S.m[r][c])) / big);
      }
    }
    CHECK(members == g.size(), "%zu members for %zu gates", members, g.size());

    // (e) the same sizes without two-qubit rotations: today's plan, and the orientation rule on top of it
    random_circuit(n, 4 + 6 * trial, false, g, th);
    std::vector<DmBlockPlan> was, now, ori;
    plan_before(n, g.data(), (int)g.size(), was);
    dm_plan_blocks(n, g.data(), (int)g.size(), now);
    dm_plan_blocks(n, g.data(), (int)g.size(), ori, DmPlanOpts{true, false});
    CHECK(was.size() == now.size() && was.size() == ori.size(), "block count changed");
    size_t gi = 0;
    for (size_t k = 0; k < was.size(); ++k) {
      CHECK(was[k].a == now[k].a && was[k].b == now[k].b && was[k].members.size() == now[k].members.size(), "block %zu changed", k);
      CHECK(ori[k].a == now[k].a && ori[k].b == now[k].b && ori[k].members.size() == now[k].members.size(), "block %zu changed by the orientation", k);
      for (size_t m = 0; m < was[k].members.size(); ++m) {
        const DmMember &x = was[k].members[m], &y = now[k].members[m], &z = ori[k].members[m];
        CHECK(x.kind == y.kind && x.pos == y.pos && x.pidx == y.pidx, "member %zu of block %zu changed", m, k);
        if (y.kind == G_DEPOL2) CHECK(y.pos == 0, "DEPOL2.pos without an override");
        CHECK(z.kind == y.kind && z.pidx == y.pidx && (y.kind == G_DEPOL2 || z.pos == y.pos), "orientation touched another member");
        ++gi;
      }
    }
    CHECK(gi == g.size(), "members lost");
    {
      // the oriented DEPOL2 members name the window position of the gate's q0.  A two-qubit gate's window is its own
      // two qubits and blocks on one window close in the order of their gates, so the gates of a window meet its
      // DEPOL2 members in order.
      const std::vector<DmBlockPlan>& chk = ori;
      long want = 0, got = 0;
      std::vector<size_t> next(chk.size(), 0);
      for (const GateRec& r : g) {
        if (r.kind != G_DEPOL2) continue;
        bool found = false;      // the first block with an unvisited DEPOL2 member on this window whose turn it is
        for (size_t k = 0; k < chk.size() && !found; ++k) {
          if (!((chk[k].a == r.q0 && chk[k].b == r.q1) || (chk[k].a == r.q1 && chk[k].b == r.q0))) continue;
          for (size_t m = next[k]; m < chk[k].members.size(); ++m) {
            if (chk[k].members[m].kind != G_DEPOL2) continue;
            const int expect = r.q0 == chk[k].a ? 0 : 1;
            CHECK(chk[k].members[m].pos == expect, "DEPOL2(%d, %d) in window (%d, %d): pos %d", r.q0, r.q1, chk[k].a, chk[k].b, chk[k].members[m].pos);
            want += expect; got += chk[k].members[m].pos;
            next[k] = m + 1;
            found = true;
            break;
          }
        }
        CHECK(found, "DEPOL2 gate without a member");
      }
      CHECK(want == got, "orientation count");
    }
  }
  CHECK(worst_c <= 1e-14, "builder chain differs from the fill by %.3e", worst_c);
  CHECK(worst_d <= 1e-13, "derivative chain differs from the exact shift by %.3e", worst_d);
  CHECK(n_rot2 > 20 && n_swapped > 5 && n_deriv > 50, "the circuits met %ld two-qubit rotations, %ld swapped channels, %ld derivatives", n_rot2, n_swapped, n_deriv);
  std::printf("blocks %ld rot2 %ld swapped %ld derivatives %ld\nkraus %.3e\nchain %.3e\nderivative %.3e\nok\n", n_blocks, n_rot2, n_swapped,
              n_deriv, worst_a, worst_c, worst_d);
  return 0;
}
