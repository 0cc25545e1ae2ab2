// dm_plan_check.cpp - CPU check of the plan / fill split of the exact channel mode (csrc/dm_host.h) and of the per-block
// builder the batched kernels compile (csrc/dm_build.h).  Host only; built by tests/test_dm_plan_cpu.py with g++.
//
// Input file: "n p1 p2 B", then per circuit "G P", G lines "kind q0 q1 pidx", P angles (hex floats).
// For every circuit:
//   (i)   dm_plan_blocks + dm_fill_blocks, and dm_make_blocks on top of them, give EXACTLY (same bits) what the
//         one-pass builder gave before the split - kept here as make_blocks_one_pass, which also counts how the
//         one-qubit gates found their window partner;
//   (ii)  dm_build_entry (members in list order, inner index ascending, identity start) gives S to <= 1e-14 per entry;
// and for the batch:
//   (iii) the flattened tables of dm_flatten_plans address every block and every member exactly once: per-circuit block
//         ranges, per-block member ranges, windows and the four window index bits ascending, channel tables.
// Prints "rules <next two-qubit gate> <free qubit> <oldest evicted>", "blocks <per circuit ...>", "maxdiff <ii>", "ok".
#include "dm_host.h"
#include "dm_build.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace vqe;

static long g_rule[3] = {0, 0, 0};

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// dm_make_blocks as it was before the plan / fill split
static void make_blocks_one_pass(int n, const GateRec* g, int G, const double* theta, double p1, double p2, std::vector<DmBlockHost>& out) {
  out.clear();
  std::vector<DmBlockHost> open;
  auto owner = [&](int q) { for (size_t k = 0; k < open.size(); ++k) if (open[k].a == q || open[k].b == q) return (int)k; return -1; };
  auto close = [&](int k) { out.push_back(open[k]); open.erase(open.begin() + k); };
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
      DmBlockHost nb{};
      nb.a = qa;
      nb.b = qb;
      if (nb.b < 0) {
        int want = -1;
        for (int j = i + 1; j < G && want < 0; ++j) {
          const bool t2 = g[j].kind == G_CNOT || g[j].kind == G_DEPOL2;
          if (t2 && g[j].q0 == qa) want = g[j].q1;
          else if (t2 && g[j].q1 == qa) want = g[j].q0;
        }
        if (want >= 0 && owner(want) < 0) { nb.b = want; ++g_rule[0]; }
        for (int q = 0; q < n && nb.b < 0; ++q) if (q != qa && owner(q) < 0) { nb.b = q; ++g_rule[1]; }
        if (nb.b < 0) { nb.b = open[0].a; close(0); ++g_rule[2]; }
      }
      sup_identity(nb.S);
      open.push_back(nb);
      k = (int)open.size() - 1;
    }
    DmBlockHost& cur = open[k];
    const int wa = cur.a;
    Sup Gs;
    if (r.kind == G_CNOT) {
      const int pc = r.q0 == wa ? 0 : 1, pt = pc ^ 1;
      cplx U[4][4];
      for (int x = 0; x < 4; ++x) for (int y = 0; y < 4; ++y) U[x][y] = (x == (y ^ (((y >> pc) & 1) << pt))) ? 1.0 : 0.0;
      sup_conj(U, Gs);
    } else if (r.kind >= G_RX && r.kind <= G_RZ) {
      const double c = std::cos(0.5 * theta[r.pidx]), sn = std::sin(0.5 * theta[r.pidx]);
      cplx R[2][2], U[4][4];
      if (r.kind == G_RX) { R[0][0] = R[1][1] = c; R[0][1] = R[1][0] = cplx(0.0, sn); }
      else if (r.kind == G_RY) { R[0][0] = R[1][1] = c; R[0][1] = sn; R[1][0] = -sn; }
      else { R[0][0] = cplx(c, sn); R[1][1] = cplx(c, -sn); R[0][1] = R[1][0] = 0.0; }
      embed_1q(R, r.q0 == wa ? 0 : 1, U);
      sup_conj(U, Gs);
    } else if (r.kind == G_DEPOL1) {
      sup_depol(r.q0 == wa ? 1 : 2, p1, Gs);
    } else {
      sup_depol(3, p2, Gs);
    }
    sup_apply(cur.S, Gs);
  }
  while (!open.empty()) close(0);
}

static void same_blocks(const std::vector<DmBlockHost>& x, const std::vector<DmBlockHost>& y, const char* what, int circuit) {
  CHECK(x.size() == y.size(), "%s: circuit %d has %zu blocks, expected %zu", what, circuit, x.size(), y.size());
  for (size_t k = 0; k < x.size(); ++k) {
    CHECK(x[k].a == y[k].a && x[k].b == y[k].b, "%s: circuit %d block %zu window (%d, %d), expected (%d, %d)", what, circuit, k,
          x[k].a, x[k].b, y[k].a, y[k].b);
    CHECK(std::memcmp(&x[k].S, &y[k].S, sizeof(Sup)) == 0, "%s: circuit %d block %zu: S differs in its bits", what, circuit, k);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: dm_plan_check <circuits file>\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::perror(argv[1]); return 2; }
  int n, B;
  double p1, p2;
  if (std::fscanf(f, "%d %la %la %d", &n, &p1, &p2, &B) != 4) return 2;
  std::vector<GateRec> gates;
  std::vector<int64_t> gbeg(B), pbeg(B);
  std::vector<int32_t> gcnt(B), pcnt(B);
  std::vector<double> theta;
  for (int b = 0; b < B; ++b) {
    int G, P;
    if (std::fscanf(f, "%d %d", &G, &P) != 2) return 2;
    gbeg[b] = (int64_t)gates.size(); gcnt[b] = G; pbeg[b] = (int64_t)theta.size(); pcnt[b] = P;
    for (int i = 0; i < G; ++i) {
      GateRec r;
      if (std::fscanf(f, "%d %d %d %d", &r.kind, &r.q0, &r.q1, &r.pidx) != 4) return 2;
      gates.push_back(r);
    }
    for (int j = 0; j < P; ++j) { double t; if (std::fscanf(f, "%la", &t) != 1) return 2; theta.push_back(t); }
  }
  std::fclose(f);

  std::vector<std::vector<DmBlockPlan>> plans(B);
  double maxdiff = 0.0;
  std::vector<double> dep;
  dm_depol_tables(p1, p2, dep);
  std::printf("blocks");
  for (int b = 0; b < B; ++b) {
    const GateRec* g = gates.data() + gbeg[b];
    const double* th = theta.data() + pbeg[b];
    std::vector<DmBlockHost> ref, made, filled;
    make_blocks_one_pass(n, g, gcnt[b], th, p1, p2, ref);
    dm_make_blocks(n, g, gcnt[b], th, p1, p2, made);
    dm_plan_blocks(n, g, gcnt[b], plans[b]);
    dm_fill_blocks(plans[b], th, p1, p2, filled);
    same_blocks(made, ref, "dm_make_blocks", b);           // (i)
    same_blocks(filled, ref, "plan + fill", b);
    std::printf(" %zu", ref.size());
    // the plan itself: every gate is a member of exactly one block, in its own order
    size_t members = 0;
    for (size_t k = 0; k < plans[b].size(); ++k) {
      const DmBlockPlan& pk = plans[b][k];
      CHECK(pk.a == ref[k].a && pk.b == ref[k].b && pk.a != pk.b && pk.a >= 0 && pk.b >= 0 && pk.a < n && pk.b < n, "plan window");
      CHECK(!pk.members.empty(), "circuit %d block %zu has no member", b, k);
      members += pk.members.size();
      for (const DmMember& m : pk.members) {
        CHECK(m.kind >= G_CNOT && m.kind <= G_DEPOL2 && (m.pos == 0 || m.pos == 1), "member kind / position");
        CHECK((m.kind >= G_RX && m.kind <= G_RZ) ? (m.pidx >= 0 && m.pidx < pcnt[b]) : m.pidx == -1, "member parameter");
      }
      // (ii) the shared builder
      double s[2][2][256];
      int cur = 0;
      for (int t = 0; t < 256; ++t) { s[0][0][t] = (t >> 4) == (t & 15) ? 1.0 : 0.0; s[0][1][t] = 0.0; }
      for (const DmMember& m : pk.members) {
        double cs = 1.0, sn = 0.0;
        if (m.kind >= G_RX && m.kind <= G_RZ) { cs = std::cos(0.5 * th[m.pidx]); sn = std::sin(0.5 * th[m.pidx]); }
        for (int t = 0; t < 256; ++t)
          dm_build_entry(m.kind, m.pos, cs, sn, dep.data(), s[cur][0], s[cur][1], t >> 4, t & 15, s[cur ^ 1][0][t], s[cur ^ 1][1][t]);
        cur ^= 1;
      }
      for (int t = 0; t < 256; ++t) {
        const cplx want = filled[k].S.m[t >> 4][t & 15];
        maxdiff = std::max(maxdiff, std::max(std::fabs(s[cur][0][t] - want.real()), std::fabs(s[cur][1][t] - want.imag())));
      }
    }
    CHECK(members == (size_t)gcnt[b], "circuit %d: %zu members for %d gates", b, members, gcnt[b]);
  }
  std::printf("\n");
  CHECK(maxdiff <= 1e-14, "shared builder differs from the fill by %.3e", maxdiff);

  // (iii) the flattened tables
  DmBatchTables T;
  dm_flatten_plans(n, B, gates.data(), gbeg.data(), gcnt.data(), p1, p2, T);
  const size_t nblk = T.blk_circ.size(), nmem = T.mem.size() / 3;
  CHECK(T.blk_begin.size() == (size_t)B + 1 && T.blk_begin[0] == 0 && (size_t)T.blk_begin[B] == nblk, "block ranges do not span the blocks");
  CHECK(T.mem_begin.size() == nblk + 1 && T.mem_begin[0] == 0 && (size_t)T.mem_begin[nblk] == nmem && T.mem.size() % 3 == 0, "member ranges do not span the members");
  CHECK(T.blk_win.size() == 6 * nblk, "window table size");
  CHECK(nmem == gates.size(), "%zu members for %zu gates", nmem, gates.size());
  std::vector<int> blk_seen(nblk, 0), mem_seen(nmem, 0);
  int max_blocks = 0;
  for (int b = 0; b < B; ++b) {
    CHECK(T.blk_begin[b] <= T.blk_begin[b + 1], "block ranges not ascending");
    CHECK((size_t)(T.blk_begin[b + 1] - T.blk_begin[b]) == plans[b].size(), "circuit %d: block count", b);
    max_blocks = std::max(max_blocks, (int)plans[b].size());
    for (int k = T.blk_begin[b]; k < T.blk_begin[b + 1]; ++k) {
      ++blk_seen[k];
      const DmBlockPlan& pk = plans[b][k - T.blk_begin[b]];
      CHECK(T.blk_circ[k] == b, "block %d belongs to circuit %d, table says %d", k, b, T.blk_circ[k]);
      const int32_t* w = T.blk_win.data() + 6 * k;
      CHECK(w[0] == pk.a && w[1] == pk.b, "block %d window", k);
      int hb[4] = {pk.a, pk.b, pk.a + n, pk.b + n};
      std::sort(hb, hb + 4);
      for (int i = 0; i < 4; ++i) CHECK(w[2 + i] == hb[i] && w[2 + i] >= 0 && w[2 + i] < 2 * n && (i == 0 || w[2 + i] > w[1 + i]), "block %d window bits", k);
      CHECK(T.mem_begin[k] <= T.mem_begin[k + 1] && (size_t)(T.mem_begin[k + 1] - T.mem_begin[k]) == pk.members.size(), "block %d member range", k);
      for (int m = T.mem_begin[k]; m < T.mem_begin[k + 1]; ++m) {
        ++mem_seen[m];
        const DmMember& pm = pk.members[m - T.mem_begin[k]];
        CHECK(T.mem[3 * m] == pm.kind && T.mem[3 * m + 1] == pm.pos && T.mem[3 * m + 2] == pm.pidx, "member %d", m);
      }
    }
  }
  for (size_t k = 0; k < nblk; ++k) CHECK(blk_seen[k] == 1, "block %zu addressed %d times", k, blk_seen[k]);
  for (size_t m = 0; m < nmem; ++m) CHECK(mem_seen[m] == 1, "member %zu addressed %d times", m, mem_seen[m]);
  CHECK(T.max_blocks == max_blocks, "max_blocks");
  CHECK(T.dep.size() == 3 * 512, "channel tables");
  for (int w = 0; w < 3; ++w) {
    Sup S;
    sup_depol(w + 1, w == 2 ? p2 : p1, S);
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c)
      CHECK(T.dep[w * 512 + r * 16 + c] == S.m[r][c].real() && T.dep[w * 512 + 256 + r * 16 + c] == S.m[r][c].imag(), "channel table %d", w);
  }
  std::printf("rules %ld %ld %ld\nmaxdiff %.3e\nok\n", g_rule[0], g_rule[1], g_rule[2], maxdiff);
  return 0;
}
