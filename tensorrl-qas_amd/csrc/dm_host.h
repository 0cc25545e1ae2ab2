// dm_host.h - host maths of the exact channel mode (vqe_dm.h): a gate list with depolarising channels becomes a
// sequence of 16 x 16 superoperator blocks on two-qubit windows of the density matrix: the plan (windows and members,
// no angles), the fill (plan + angles -> matrices) and the flattened tables of the batched path.  Host only, no HIP.
#pragma once
#include "vqe_geo.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

namespace vqe {

typedef std::complex<double> cplx;
struct Sup { cplx m[16][16]; };      // superoperator on the window: entry index e = i + 4 j, i = ket bits (a, b), j = bra bits

inline void sup_identity(Sup& S) {
  for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) S.m[r][c] = r == c ? 1.0 : 0.0;
}
// rho -> U rho U^+ :  S[(i, j), (i', j')] = U[i][i'] conj(U[j][j'])
inline void sup_conj(const cplx U[4][4], Sup& S) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) for (int ip = 0; ip < 4; ++ip) for (int jp = 0; jp < 4; ++jp)
    S.m[i + 4 * j][ip + 4 * jp] = U[i][ip] * std::conj(U[j][jp]);
}
inline void sup_apply(Sup& acc, const Sup& G) {      // acc <- G acc
  Sup t;
  for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
    cplx v = 0.0;
    for (int k = 0; k < 16; ++k) v += G.m[r][k] * acc.m[k][c];
    t.m[r][c] = v;
  }
  acc = t;
}
// one-qubit operator on window position pos (0: qubit a = bit 0 of the 2-bit index, 1: qubit b)
inline void embed_1q(const cplx R[2][2], int pos, cplx U[4][4]) {
  for (int i = 0; i < 4; ++i) for (int ip = 0; ip < 4; ++ip) {
    const int other = pos ^ 1;
    U[i][ip] = (((i >> other) & 1) == ((ip >> other) & 1)) ? R[(i >> pos) & 1][(ip >> pos) & 1] : cplx(0.0);
  }
}
inline void pauli_1q(int p, cplx R[2][2]) {          // 0 I, 1 X, 2 Y, 3 Z
  R[0][0] = R[0][1] = R[1][0] = R[1][1] = 0.0;
  if (p == 0) { R[0][0] = R[1][1] = 1.0; }
  else if (p == 1) { R[0][1] = R[1][0] = 1.0; }
  else if (p == 2) { R[0][1] = cplx(0.0, -1.0); R[1][0] = cplx(0.0, 1.0); }
  else { R[0][0] = 1.0; R[1][1] = -1.0; }
}
// (1 - p) id + p / (4^k - 1) sum over the non-identity Paulis on the qubits of `mask` (bit 0: a, bit 1: b)
inline void sup_depol(int mask, double p, Sup& S) {
  const int k = (mask & 1) + ((mask >> 1) & 1);
  const double w = p / (k == 2 ? 15.0 : 3.0);
  for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) S.m[r][c] = r == c ? 1.0 - p : 0.0;
  for (int pa = 0; pa < 4; ++pa) for (int pb = 0; pb < 4; ++pb) {
    if ((pa && !(mask & 1)) || (pb && !(mask & 2)) || (!pa && !pb)) continue;
    cplx Ra[2][2], Rb[2][2], Ua[4][4], Ub[4][4], U[4][4];
    pauli_1q(pa, Ra); pauli_1q(pb, Rb);
    embed_1q(Ra, 0, Ua); embed_1q(Rb, 1, Ub);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
      cplx v = 0.0;
      for (int m = 0; m < 4; ++m) v += Ua[i][m] * Ub[m][j];
      U[i][j] = v;
    }
    Sup P;
    sup_conj(U, P);
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) S.m[r][c] += w * P.m[r][c];
  }
}

struct DmBlockHost { int a, b; Sup S; };

// One gate or channel inside a block.  pos: the window position (0: qubit a, 1: qubit b) a rotation or a one-qubit
// channel acts on; the position of the CONTROL for a CNOT; 0 for the two-qubit channel.  pidx: the rotation's parameter.
struct DmMember { int kind, pos, pidx; };
struct DmBlockPlan { int a, b; std::vector<DmMember> members; };

// Gate list -> blocks, WITHOUT the angles: the windows, the block every gate joins and the order in which blocks close
// follow from the gate list alone.  A block collects the gates / channels that stay inside its two-qubit window; blocks
// on DISJOINT windows commute (they act on different index bits of rho), so several blocks are open at a time and a
// gate joins the open block that holds all of its qubits wherever that block was opened; a gate that touches an open
// window without fitting into it closes that block first (blocks are emitted in the order they are closed, which keeps
// every qubit's own sequence of operations intact).  Bench circuits (63 gates + 63 channels on 12 qubits): 57 blocks
// with consecutive fusion only, ~40 with this one.
inline void dm_plan_blocks(int n, const GateRec* g, int G, std::vector<DmBlockPlan>& out) {
  out.clear();
  std::vector<DmBlockPlan> open;            // pairwise disjoint windows
  auto owner = [&](int q) { for (size_t k = 0; k < open.size(); ++k) if (open[k].a == q || open[k].b == q) return (int)k; return -1; };
  auto close = [&](int k) { out.push_back(std::move(open[k])); open.erase(open.begin() + k); };
  for (int i = 0; i < G; ++i) {
    const GateRec r = g[i];
    const bool two = r.kind == G_CNOT || r.kind == G_DEPOL2;
    const int qa = r.q0, qb = two ? r.q1 : -1;
    int k = owner(qa);
    const int k2 = two ? owner(qb) : k;
    if (k < 0 || k2 != k) {
      // no open block holds all qubits of the gate: close the ones it touches (the higher index first), open a new one
      const int c1 = k, c2 = two ? k2 : -1;
      if (c1 >= 0 && c2 >= 0 && c1 != c2) { close(std::max(c1, c2)); close(std::min(c1, c2)); }
      else if (c1 >= 0) close(c1);
      else if (c2 >= 0) close(c2);
      DmBlockPlan nb{};
      nb.a = qa;
      nb.b = qb;
      if (nb.b < 0) {
        // a one-qubit gate opens the window: its partner is the other qubit of the next two-qubit gate that touches it,
        // if that qubit is free; else any free qubit; if every other qubit sits in an open window, the oldest block goes
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

// Plan + angles + channel strengths -> the superoperators: identity, then the members in list order.  Gate semantics as
// in vqe_device.h (qulacs: R = exp(+i theta/2 P), CNOT(control, target)).
inline void dm_fill_blocks(const std::vector<DmBlockPlan>& plan, const double* theta, double p1, double p2, std::vector<DmBlockHost>& out) {
  out.clear();
  out.reserve(plan.size());
  for (const DmBlockPlan& b : plan) {
    out.push_back(DmBlockHost{});
    DmBlockHost& cur = out.back();
    cur.a = b.a;
    cur.b = b.b;
    sup_identity(cur.S);
    for (const DmMember& m : b.members) {
      Sup Gs;
      if (m.kind == G_CNOT) {
        const int pc = m.pos, pt = pc ^ 1;
        cplx U[4][4];
        for (int x = 0; x < 4; ++x) for (int y = 0; y < 4; ++y) U[x][y] = (x == (y ^ (((y >> pc) & 1) << pt))) ? 1.0 : 0.0;
        sup_conj(U, Gs);
      } else if (m.kind >= G_RX && m.kind <= G_RZ) {
        const double c = std::cos(0.5 * theta[m.pidx]), sn = std::sin(0.5 * theta[m.pidx]);
        cplx R[2][2], U[4][4];
        if (m.kind == G_RX) { R[0][0] = R[1][1] = c; R[0][1] = R[1][0] = cplx(0.0, sn); }
        else if (m.kind == G_RY) { R[0][0] = R[1][1] = c; R[0][1] = sn; R[1][0] = -sn; }
        else { R[0][0] = cplx(c, sn); R[1][1] = cplx(c, -sn); R[0][1] = R[1][0] = 0.0; }
        embed_1q(R, m.pos, U);
        sup_conj(U, Gs);
      } else if (m.kind == G_DEPOL1) {
        sup_depol(m.pos == 0 ? 1 : 2, p1, Gs);
      } else {
        sup_depol(3, p2, Gs);
      }
      sup_apply(cur.S, Gs);
    }
  }
}

// Gate list -> superoperator blocks: the plan, filled.
inline void dm_make_blocks(int n, const GateRec* g, int G, const double* theta, double p1, double p2, std::vector<DmBlockHost>& out) {
  std::vector<DmBlockPlan> plan;
  dm_plan_blocks(n, g, G, plan);
  dm_fill_blocks(plan, theta, p1, p2, out);
}

// ---- the batched path (vqe_dm_batch.h): the plans of a resident batch, flattened for the device -------------------
// blk_begin[b] .. blk_begin[b + 1]: the blocks of circuit b in sweep order; block k: circuit blk_circ[k], window
// blk_win[6 k] = a, [6 k + 1] = b, [6 k + 2 .. 6 k + 5] = the four index bits of the window in rho (a, b, a + n, b + n)
// ascending; its members mem[3 m] = kind, [3 m + 1] = pos, [3 m + 2] = pidx for m in mem_begin[k] .. mem_begin[k + 1].
// dep: the three channel superoperators [which][re / im][16][16] (which 0: one-qubit channel on window position 0,
// 1: on position 1, 2: the two-qubit channel), from sup_depol - they depend on p1 / p2 only.
struct DmBatchTables {
  std::vector<int32_t> blk_begin, blk_circ, blk_win, mem_begin, mem;
  std::vector<double> dep;
  int max_blocks = 0;      // the largest block count of a circuit (levels of an evaluation)
};
inline void dm_depol_tables(double p1, double p2, std::vector<double>& dep) {
  dep.assign(3 * 512, 0.0);
  for (int w = 0; w < 3; ++w) {
    Sup S;
    sup_depol(w + 1, w == 2 ? p2 : p1, S);
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
      dep[w * 512 + r * 16 + c] = S.m[r][c].real();
      dep[w * 512 + 256 + r * 16 + c] = S.m[r][c].imag();
    }
  }
}
inline void dm_flatten_plans(int n, int batch, const GateRec* gates, const int64_t* gate_begin, const int32_t* gate_count,
                             double p1, double p2, DmBatchTables& T) {
  T = DmBatchTables{};
  T.blk_begin.push_back(0);
  T.mem_begin.push_back(0);
  std::vector<DmBlockPlan> plan;
  for (int b = 0; b < batch; ++b) {
    dm_plan_blocks(n, gates + gate_begin[b], gate_count[b], plan);
    for (const DmBlockPlan& k : plan) {
      int hb[4] = {k.a, k.b, k.a + n, k.b + n};
      std::sort(hb, hb + 4);
      T.blk_circ.push_back(b);
      T.blk_win.insert(T.blk_win.end(), {k.a, k.b, hb[0], hb[1], hb[2], hb[3]});
      for (const DmMember& m : k.members) T.mem.insert(T.mem.end(), {m.kind, m.pos, m.pidx});
      T.mem_begin.push_back((int32_t)(T.mem.size() / 3));
    }
    T.blk_begin.push_back((int32_t)T.blk_circ.size());
    T.max_blocks = std::max(T.max_blocks, (int)plan.size());
  }
  dm_depol_tables(p1, p2, T.dep);
}

// ---- the adjoint gradient of the batched path (vqe_dm_grad.h) ------------------------------------------------------
// A gradient evaluation keeps rho_0 .. rho_L and Lambda of every resident circuit: levels + 2 density matrices.  The
// circuits resident at a time for a budget of `budget_bytes` (max_resident density matrices, or a quarter of the free
// memory - the budget of an energy run): 0 when not even one fits, never more than the batch or the y extent of a grid.
inline int dm_grad_resident(size_t budget_bytes, int n, int levels, int batch) {
  const size_t per_circuit = ((size_t)levels + 2) * (sizeof(double) * 2 << (2 * n));
  return (int)std::min<size_t>(std::min<size_t>(budget_bytes / per_circuit, (size_t)std::max(batch, 0)), 65535);
}
// The groups of 16 window entries of a level are summed into M in tiles of 16 groups; a partial sum covers
// dm_grad_tiles_per_partial(n) consecutive tiles, a function of n alone: at most 256 partials, 4 tiles or more each.
inline uint32_t dm_grad_tiles(int n) { return (uint32_t)(((((size_t)1 << (2 * n)) / 16) + 15) / 16); }
inline uint32_t dm_grad_tiles_per_partial(int n) { return std::max<uint32_t>(4u, (dm_grad_tiles(n) + 255u) / 256u); }
inline uint32_t dm_grad_partials(int n) { return (dm_grad_tiles(n) + dm_grad_tiles_per_partial(n) - 1u) / dm_grad_tiles_per_partial(n); }

}  // namespace vqe
