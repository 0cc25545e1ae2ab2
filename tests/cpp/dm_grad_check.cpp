// dm_grad_check.cpp - CPU check of the adjoint gradient of the batched exact channel mode (csrc/vqe_dm_grad.h, DESIGN
// 4.13): the derivative chain of csrc/dm_build.h, the whole formula on the host, the memory rule of csrc/dm_host.h.
// Host only; built by tests/test_dm_grad_cpu.py with g++.
//
//   dm_grad_check chain <file>      per circuit, block and rotation member: dm_block_derivative against the exact shift
//                                   (S(theta + pi/2) - S(theta - pi/2)) / 2 of dm_fill_blocks, per entry, relative to the
//                                   block's largest entry.  Every rotation has an angle of its own.  Prints "chain <max>".
//   dm_grad_check formula <file>    (n <= 4) a plain host loop applies the blocks with rho_0 .. rho_L kept, forms
//                                   Lambda_L = conj(h), M_l, the contraction with dm_block_derivative and Lambda_{l-1} =
//                                   S_l^+ Lambda_l - the formula the kernels implement - against the parameter shift of
//                                   the host energy.  State and Hamiltonian (complex coefficients) come from a fixed
//                                   generator.  Prints "formula <max |difference|>".
//   dm_grad_check resident <budget bytes> <n> <levels> <batch>     prints dm_grad_resident(...)
//   dm_grad_check partials <n>                                     prints "<tiles> <tiles per partial> <partials>"
// File: "n p1 p2 B", then per circuit "G P", G lines "kind q0 q1 pidx", P angles (hex floats) - dm_plan_check's format.
#include "dm_host.h"
#include "dm_build.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace vqe;

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static const double kHalfPi = 1.57079632679489661923;

struct Batch {
  int n = 0, B = 0;
  double p1 = 0, p2 = 0;
  std::vector<GateRec> gates;
  std::vector<int64_t> gbeg, pbeg;
  std::vector<int32_t> gcnt, pcnt;
  std::vector<double> theta;
};

static bool read_batch(const char* path, Batch& b) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) { std::perror(path); return false; }
  if (std::fscanf(f, "%d %la %la %d", &b.n, &b.p1, &b.p2, &b.B) != 4) return false;
  b.gbeg.resize(b.B); b.pbeg.resize(b.B); b.gcnt.resize(b.B); b.pcnt.resize(b.B);
  for (int c = 0; c < b.B; ++c) {
    int G, P;
    if (std::fscanf(f, "%d %d", &G, &P) != 2) return false;
    b.gbeg[c] = (int64_t)b.gates.size(); b.gcnt[c] = G; b.pbeg[c] = (int64_t)b.theta.size(); b.pcnt[c] = P;
    for (int i = 0; i < G; ++i) {
      GateRec r;
      if (std::fscanf(f, "%d %d %d %d", &r.kind, &r.q0, &r.q1, &r.pidx) != 4) return false;
      b.gates.push_back(r);
    }
    for (int j = 0; j < P; ++j) { double t; if (std::fscanf(f, "%la", &t) != 1) return false; b.theta.push_back(t); }
  }
  std::fclose(f);
  return true;
}

// dS/dtheta of block `blk` for its member `which` through dm_block_derivative -> Sup
static void derivative(const DmBlockPlan& blk, int which, const double* th, const std::vector<double>& dep, Sup& out) {
  const int k = (int)blk.members.size();
  std::vector<int32_t> mem;
  std::vector<double> cs(k, 1.0), sn(k, 0.0);
  for (int m = 0; m < k; ++m) {
    const DmMember& d = blk.members[m];
    mem.insert(mem.end(), {d.kind, d.pos, d.pidx});
    if (d.kind >= G_RX && d.kind <= G_RZ) { cs[m] = std::cos(0.5 * th[d.pidx]); sn[m] = std::sin(0.5 * th[d.pidx]); }
  }
  double o[2][256], t[2][256];
  dm_block_derivative(mem.data(), k, which, cs.data(), sn.data(), dep.data(), o[0], o[1], t[0], t[1]);
  for (int e = 0; e < 256; ++e) out.m[e >> 4][e & 15] = cplx(o[0][e], o[1][e]);
}

static int run_chain(const Batch& b) {
  std::vector<double> dep;
  dm_depol_tables(b.p1, b.p2, dep);
  double worst = 0.0;
  long checked = 0;
  for (int c = 0; c < b.B; ++c) {
    std::vector<DmBlockPlan> plan;
    dm_plan_blocks(b.n, b.gates.data() + b.gbeg[c], b.gcnt[c], plan);
    std::vector<double> th(b.theta.begin() + b.pbeg[c], b.theta.begin() + b.pbeg[c] + b.pcnt[c]);
    std::vector<int> uses(b.pcnt[c], 0);
    for (const DmBlockPlan& k : plan) for (const DmMember& m : k.members) if (m.pidx >= 0) ++uses[m.pidx];
    for (int u : uses) CHECK(u <= 1, "circuit %d: a parameter is shared; the chain check wants private angles", c);
    std::vector<DmBlockHost> at, up, dn;
    dm_fill_blocks(plan, th.data(), b.p1, b.p2, at);
    for (size_t k = 0; k < plan.size(); ++k) {
      double scale = 0.0;
      for (int r = 0; r < 16; ++r) for (int cc = 0; cc < 16; ++cc) scale = std::max(scale, std::abs(at[k].S.m[r][cc]));
      for (size_t m = 0; m < plan[k].members.size(); ++m) {
        const DmMember& d = plan[k].members[m];
        if (d.kind < G_RX || d.kind > G_RZ) continue;
        Sup dS;
        derivative(plan[k], (int)m, th.data(), dep, dS);
        std::vector<DmBlockPlan> one(1, plan[k]);
        const double keep = th[d.pidx];
        th[d.pidx] = keep + kHalfPi; dm_fill_blocks(one, th.data(), b.p1, b.p2, up);
        th[d.pidx] = keep - kHalfPi; dm_fill_blocks(one, th.data(), b.p1, b.p2, dn);
        th[d.pidx] = keep;
        for (int r = 0; r < 16; ++r) for (int cc = 0; cc < 16; ++cc)
          worst = std::max(worst, std::abs(dS.m[r][cc] - 0.5 * (up[0].S.m[r][cc] - dn[0].S.m[r][cc])) / scale);
        ++checked;
      }
    }
  }
  std::printf("members %ld\nchain %.3e\n", checked, worst);
  CHECK(worst <= 1e-14, "derivative chain differs from the exact shift by %.3e of the block's largest entry", worst);
  std::printf("ok\n");
  return 0;
}

// ---- the whole formula on the host -------------------------------------------------------------------------------
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static double uniform() {      // splitmix64 -> (-1, 1)
  uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) / 4503599627370496.0 - 1.0;
}

// the 16 entries of group g of window (a, b): entry e has ket bits (e & 1, e >> 1 & 1) at a, b and bra bits at a + n, b + n
static void group_index(int n, int a, int b, uint32_t g, uint32_t idx[16]) {
  int hb[4] = {a, b, a + n, b + n};
  std::sort(hb, hb + 4);
  uint32_t base = g;
  for (int i = 0; i < 4; ++i) base = ((base >> hb[i]) << (hb[i] + 1)) | (base & ((1u << hb[i]) - 1u));
  for (uint32_t e = 0; e < 16; ++e)
    idx[e] = base | ((e & 1u) << a) | (((e >> 1) & 1u) << b) | (((e >> 2) & 1u) << (a + n)) | (((e >> 3) & 1u) << (b + n));
}
static void apply_block(int n, const DmBlockHost& blk, bool adjoint, std::vector<cplx>& v) {
  const uint32_t groups = (uint32_t)(v.size() / 16);
  for (uint32_t g = 0; g < groups; ++g) {
    uint32_t idx[16];
    group_index(n, blk.a, blk.b, g, idx);
    cplx in[16];
    for (int e = 0; e < 16; ++e) in[e] = v[idx[e]];
    for (int r = 0; r < 16; ++r) {
      cplx s = 0.0;
      for (int c = 0; c < 16; ++c) s += (adjoint ? std::conj(blk.S.m[c][r]) : blk.S.m[r][c]) * in[c];
      v[idx[r]] = s;
    }
  }
}
static double host_energy(int n, const std::vector<DmBlockPlan>& plan, const double* th, double p1, double p2, const std::vector<cplx>& rho0,
                          const std::vector<cplx>& h) {
  std::vector<DmBlockHost> blocks;
  dm_fill_blocks(plan, th, p1, p2, blocks);
  std::vector<cplx> rho = rho0;
  for (const DmBlockHost& k : blocks) apply_block(n, k, false, rho);
  double e = 0.0;
  for (size_t f = 0; f < rho.size(); ++f) e += (h[f] * rho[f]).real();
  return e;
}

static int run_formula(const Batch& b) {
  const int n = b.n;
  CHECK(n >= 2 && n <= 4, "the host formula runs at n = 2, 3, 4");
  const uint32_t dim = 1u << n;
  const size_t total = (size_t)dim * dim;
  std::vector<double> dep;
  dm_depol_tables(b.p1, b.p2, dep);
  // |psi><psi| and h: h[i | (i ^ x) << n] += +-c, the sign from popc(i & z); complex coefficients, distinct X masks
  // per group as the engine groups them (several terms may share an X mask)
  std::vector<cplx> psi(dim), rho0(total), h(total, 0.0);
  double nrm = 0.0;
  for (cplx& a : psi) { a = cplx(uniform(), uniform()); nrm += std::norm(a); }
  for (cplx& a : psi) a /= std::sqrt(nrm);
  for (uint32_t i = 0; i < dim; ++i) for (uint32_t j = 0; j < dim; ++j) rho0[(size_t)i | ((size_t)j << n)] = psi[i] * std::conj(psi[j]);
  double csum = 0.0;
  for (int t = 0; t < 3 * n + 2; ++t) {
    const uint32_t x = (uint32_t)((uniform() + 1.0) * 0.5 * dim) & (dim - 1), z = (uint32_t)((uniform() + 1.0) * 0.5 * dim) & (dim - 1);
    const cplx c(uniform(), 0.3 * uniform());
    csum += std::abs(c);
    for (uint32_t i = 0; i < dim; ++i) h[(size_t)i | ((size_t)(i ^ x) << n)] += (__builtin_popcount(i & z) & 1) ? -c : c;
  }
  double worst = 0.0;
  long checked = 0;
  for (int c = 0; c < b.B; ++c) {
    std::vector<DmBlockPlan> plan;
    dm_plan_blocks(n, b.gates.data() + b.gbeg[c], b.gcnt[c], plan);
    std::vector<double> th(b.theta.begin() + b.pbeg[c], b.theta.begin() + b.pbeg[c] + b.pcnt[c]);
    const int P = b.pcnt[c], L = (int)plan.size();
    std::vector<int> uses(P, 0);
    for (const DmBlockPlan& k : plan) for (const DmMember& m : k.members) if (m.pidx >= 0) ++uses[m.pidx];
    for (int u : uses) CHECK(u <= 1, "circuit %d: a shared parameter has no two-term shift rule", c);
    std::vector<DmBlockHost> blocks;
    dm_fill_blocks(plan, th.data(), b.p1, b.p2, blocks);
    std::vector<std::vector<cplx>> rho(L + 1);
    rho[0] = rho0;
    for (int l = 0; l < L; ++l) { rho[l + 1] = rho[l]; apply_block(n, blocks[l], false, rho[l + 1]); }
    std::vector<cplx> lam(total);
    for (size_t f = 0; f < total; ++f) lam[f] = std::conj(h[f]);
    std::vector<double> grad(P, 0.0);
    for (int l = L - 1; l >= 0; --l) {      // block l: rho[l] beside Lambda_{l+1}
      cplx M[16][16];
      for (int r = 0; r < 16; ++r) for (int cc = 0; cc < 16; ++cc) M[r][cc] = 0.0;
      for (uint32_t g = 0; g < total / 16; ++g) {
        uint32_t idx[16];
        group_index(n, blocks[l].a, blocks[l].b, g, idx);
        for (int r = 0; r < 16; ++r) for (int cc = 0; cc < 16; ++cc) M[r][cc] += std::conj(lam[idx[r]]) * rho[l][idx[cc]];
      }
      for (size_t m = 0; m < plan[l].members.size(); ++m) {
        const DmMember& d = plan[l].members[m];
        if (d.kind < G_RX || d.kind > G_RZ) continue;
        Sup dS;
        derivative(plan[l], (int)m, th.data(), dep, dS);
        double v = 0.0;
        for (int r = 0; r < 16; ++r) for (int cc = 0; cc < 16; ++cc) v += (dS.m[r][cc] * M[r][cc]).real();
        grad[d.pidx] += v;
      }
      apply_block(n, blocks[l], true, lam);
    }
    for (int p = 0; p < P; ++p) {
      const double keep = th[p];
      th[p] = keep + kHalfPi; const double up = host_energy(n, plan, th.data(), b.p1, b.p2, rho0, h);
      th[p] = keep - kHalfPi; const double dn = host_energy(n, plan, th.data(), b.p1, b.p2, rho0, h);
      th[p] = keep;
      worst = std::max(worst, std::fabs(grad[p] - 0.5 * (up - dn)));
      ++checked;
      if (!uses[p]) CHECK(grad[p] == 0.0, "an unused parameter has gradient %.3e", grad[p]);
    }
  }
  std::printf("parameters %ld\ncoefficients %.6f\nformula %.3e\n", checked, csum, worst);
  CHECK(worst <= 1e-12, "host formula differs from the parameter shift by %.3e", worst);
  std::printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 6 && !std::strcmp(argv[1], "resident")) {
    std::printf("%d\n", dm_grad_resident((size_t)std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5])));
    return 0;
  }
  if (argc >= 3 && !std::strcmp(argv[1], "partials")) {
    const int n = std::atoi(argv[2]);
    std::printf("%u %u %u\n", dm_grad_tiles(n), dm_grad_tiles_per_partial(n), dm_grad_partials(n));
    return 0;
  }
  if (argc < 3) { std::fprintf(stderr, "usage: dm_grad_check chain|formula <circuits file> | resident <budget> <n> <levels> <batch> | partials <n>\n"); return 2; }
  Batch b;
  if (!read_batch(argv[2], b)) return 2;
  if (!std::strcmp(argv[1], "chain")) return run_chain(b);
  if (!std::strcmp(argv[1], "formula")) return run_formula(b);
  return 2;
}
