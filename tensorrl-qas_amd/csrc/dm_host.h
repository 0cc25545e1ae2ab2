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

// A Kraus set in the place of a depolarising channel (vqe_set_noise_kraus): rho -> sum_k K_k rho K_k^+.
// One-qubit operators K[k][2][2] on window position pos.
inline void sup_kraus_1q(const cplx* K, int n1, int pos, Sup& S) {
  for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) S.m[r][c] = 0.0;
  for (int k = 0; k < n1; ++k) {
    cplx R[2][2] = {{K[4 * k], K[4 * k + 1]}, {K[4 * k + 2], K[4 * k + 3]}}, U[4][4];
    embed_1q(R, pos, U);
    Sup P;
    sup_conj(U, P);
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) S.m[r][c] += P.m[r][c];
  }
}
// Two-qubit operators K[k][4][4], basis index = bit(q0) + 2 bit(q1) of the GATE's qubits.  swapped: the gate's q0 sits on
// window position 1 (qubit b), so the two bits of every index change places on the way into the window.
inline void sup_kraus_2q(const cplx* K, int n2, bool swapped, Sup& S) {
  for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) S.m[r][c] = 0.0;
  for (int k = 0; k < n2; ++k) {
    cplx U[4][4];
    for (int i = 0; i < 4; ++i) for (int ip = 0; ip < 4; ++ip) {
      const int gi = swapped ? ((i & 1) << 1) | (i >> 1) : i, gp = swapped ? ((ip & 1) << 1) | (ip >> 1) : ip;
      U[i][ip] = K[16 * k + 4 * gi + gp];
    }
    Sup P;
    sup_conj(U, P);
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) S.m[r][c] += P.m[r][c];
  }
}
// The override of a handle: K1 (n1 x 2 x 2) replaces the channel of G_DEPOL1, K2 (n2 x 4 x 4) that of G_DEPOL2; a count
// of 0 leaves that slot on the depolarising channel.
struct DmKraus {
  int n1 = 0, n2 = 0;
  std::vector<cplx> K1, K2;
  bool any() const { return n1 > 0 || n2 > 0; }
};
// max |sum_k K_k^+ K_k - I| of `count` d x d operators: 0 for a trace preserving set, NaN if an entry is no number
inline double kraus_tp_defect(const cplx* K, int count, int d) {
  double worst = 0.0;
  for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) {
    cplx v = r == c ? -1.0 : 0.0;
    for (int k = 0; k < count; ++k) for (int m = 0; m < d; ++m) v += std::conj(K[(k * d + m) * d + r]) * K[(k * d + m) * d + c];
    const double a = std::abs(v);
    if (a != a) return a;      // (std::max would drop it)
    worst = std::max(worst, a);
  }
  return worst;
}
// The Kraus set of a Pauli channel (vqe_set_noise_pauli): sqrt(w_0) 1 first, w_0 = 1 - (w_1 + ... + w_m) summed in this
// order and not below 0, then sqrt(w_k) P_k at k = 1 .. m: X, Y, Z for d = 2; P_b (x) P_a at k = a + 4 b for d = 4 (P_a on
// q0, the low index bit) - the order of the depolarising set of vqe_set_kraus_traj.  4 or 16 operators; a zero weight
// leaves a zero operator, which no trajectory selects and which adds nothing to a superoperator.
inline void pauli_kraus(const double* w, int d, std::vector<cplx>& K) {
  const int m = d == 2 ? 3 : 15;
  double tot = 0.0;
  for (int k = 0; k < m; ++k) tot += w[k];
  K.clear();
  for (int b = 0; b < (d == 2 ? 1 : 4); ++b) for (int a = 0; a < 4; ++a) {
    const int k = a + 4 * b;
    const double s = std::sqrt(k ? w[k - 1] : std::max(0.0, 1.0 - tot));
    cplx Ra[2][2], Rb[2][2];
    pauli_1q(a, Ra); pauli_1q(b, Rb);
    for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c)
      K.push_back(d == 2 ? s * Ra[r][c] : s * Ra[r & 1][c & 1] * Rb[r >> 1][c >> 1]);
  }
}
// What the plan depends on beside the gate list.  orient2: a two-qubit Kraus set is installed, so a G_DEPOL2 member
// carries the window position of the gate's q0 (depolarising noise is symmetric under exchange of its qubits: pos 0).
// rot2: RXX / RYY / RZZ are window-sized members like a CNOT (vqe_set_dm_rot2).
struct DmPlanOpts { bool orient2 = false, rot2 = false; };

struct DmBlockHost { int a, b; Sup S; };

// One gate or channel inside a block.  pos: the window position (0: qubit a, 1: qubit b) a rotation or a one-qubit
// channel acts on; the position of the CONTROL for a CNOT and of q0 for a two-qubit rotation; for the two-qubit channel
// 0, or the position of q0 when a two-qubit Kraus set is installed (DmPlanOpts).  pidx: the rotation's parameter.
struct DmMember { int kind, pos, pidx; };
struct DmBlockPlan { int a, b; std::vector<DmMember> members; };

// Gate list -> blocks, WITHOUT the angles: the windows, the block every gate joins and the order in which blocks close
// follow from the gate list alone.  A block collects the gates / channels that stay inside its two-qubit window; blocks
// on DISJOINT windows commute (they act on different index bits of rho), so several blocks are open at a time and a
// gate joins the open block that holds all of its qubits wherever that block was opened; a gate that touches an open
// window without fitting into it closes that block first (blocks are emitted in the order they are closed, which keeps
// every qubit's own sequence of operations intact).  Bench circuits (63 gates + 63 channels on 12 qubits): 57 blocks
// with consecutive fusion only, ~40 with this one.
inline void dm_plan_blocks(int n, const GateRec* g, int G, std::vector<DmBlockPlan>& out, DmPlanOpts opt = DmPlanOpts{}) {
  out.clear();
  const auto is_two = [&](int kind) { return kind == G_CNOT || kind == G_DEPOL2 || (opt.rot2 && gate_is_rot2(kind)); };
  std::vector<DmBlockPlan> open;            // pairwise disjoint windows
  auto owner = [&](int q) { for (size_t k = 0; k < open.size(); ++k) if (open[k].a == q || open[k].b == q) return (int)k; return -1; };
  auto close = [&](int k) { out.push_back(std::move(open[k])); open.erase(open.begin() + k); };
  for (int i = 0; i < G; ++i) {
    const GateRec r = g[i];
    const bool two = is_two(r.kind);
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
          const bool t2 = is_two(g[j].kind);
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
    cur.members.push_back(DmMember{r.kind, (r.kind == G_DEPOL2 && !opt.orient2) ? 0 : pos, gate_is_rot(r.kind) ? r.pidx : -1});
  }
  while (!open.empty()) close(0);
}

// Plan + angles + channel strengths -> the superoperators: identity, then the members in list order.  Gate semantics as
// in vqe_device.h (qulacs: R = exp(+i theta/2 P), CNOT(control, target)).  kr: the Kraus override, or NULL.
inline void dm_fill_blocks(const std::vector<DmBlockPlan>& plan, const double* theta, double p1, double p2, std::vector<DmBlockHost>& out,
                           const DmKraus* kr = nullptr) {
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
      } else if (gate_is_rot2(m.kind)) {      // U = cos(theta/2) I + i sin(theta/2) P (x) P on the window
        const double c = std::cos(0.5 * theta[m.pidx]), sn = std::sin(0.5 * theta[m.pidx]);
        cplx R[2][2], Ua[4][4], Ub[4][4], U[4][4];
        pauli_1q(m.kind - G_RXX + 1, R);
        embed_1q(R, 0, Ua); embed_1q(R, 1, Ub);
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
          cplx v = 0.0;
          for (int k = 0; k < 4; ++k) v += Ua[i][k] * Ub[k][j];
          U[i][j] = (i == j ? cplx(c) : cplx(0.0)) + cplx(0.0, sn) * v;
        }
        sup_conj(U, Gs);
      } else if (m.kind == G_DEPOL1) {
        if (kr && kr->n1) sup_kraus_1q(kr->K1.data(), kr->n1, m.pos, Gs);
        else sup_depol(m.pos == 0 ? 1 : 2, p1, Gs);
      } else {
        if (kr && kr->n2) sup_kraus_2q(kr->K2.data(), kr->n2, m.pos == 1, Gs);
        else sup_depol(3, p2, Gs);
      }
      sup_apply(cur.S, Gs);
    }
  }
}

// Gate list -> superoperator blocks: the plan, filled.
inline void dm_make_blocks(int n, const GateRec* g, int G, const double* theta, double p1, double p2, std::vector<DmBlockHost>& out,
                           const DmKraus* kr = nullptr, bool rot2 = false) {
  std::vector<DmBlockPlan> plan;
  dm_plan_blocks(n, g, G, plan, DmPlanOpts{kr && kr->n2 > 0, rot2});
  dm_fill_blocks(plan, theta, p1, p2, out, kr);
}

// ---- the batched path (vqe_dm_batch.h): the plans of a resident batch, flattened for the device -------------------
// blk_begin[b] .. blk_begin[b + 1]: the blocks of circuit b in sweep order; block k: circuit blk_circ[k], window
// blk_win[6 k] = a, [6 k + 1] = b, [6 k + 2 .. 6 k + 5] = the four index bits of the window in rho (a, b, a + n, b + n)
// ascending; its members mem[3 m] = kind, [3 m + 1] = pos, [3 m + 2] = pidx for m in mem_begin[k] .. mem_begin[k + 1].
// dep: the three channel superoperators [which][re / im][16][16] (which 0: one-qubit channel on window position 0,
// 1: on position 1, 2: the two-qubit channel), from sup_depol - they depend on p1 / p2 only.  With a Kraus override
// (dm_channel_tables) FOUR slices: 2 = the two-qubit channel with the gate's q0 on window position 0, 3 = with q0 on
// position 1; a member reads slice 2 + pos, and without a two-qubit Kraus set pos is 0, so slice 3 is never read.
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
// the four slices: every slot from its Kraus set where one is installed, else from sup_depol
inline void dm_channel_tables(double p1, double p2, const DmKraus* kr, std::vector<double>& dep) {
  dep.assign(4 * 512, 0.0);
  for (int w = 0; w < 4; ++w) {
    Sup S;
    if (w < 2) { if (kr && kr->n1) sup_kraus_1q(kr->K1.data(), kr->n1, w, S); else sup_depol(w + 1, p1, S); }
    else if (kr && kr->n2) sup_kraus_2q(kr->K2.data(), kr->n2, w == 3, S);
    else sup_depol(3, p2, S);
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
      dep[w * 512 + r * 16 + c] = S.m[r][c].real();
      dep[w * 512 + 256 + r * 16 + c] = S.m[r][c].imag();
    }
  }
}
inline void dm_flatten_plans(int n, int batch, const GateRec* gates, const int64_t* gate_begin, const int32_t* gate_count,
                             double p1, double p2, DmBatchTables& T, const DmKraus* kr = nullptr, bool rot2 = false) {
  T = DmBatchTables{};
  T.blk_begin.push_back(0);
  T.mem_begin.push_back(0);
  std::vector<DmBlockPlan> plan;
  for (int b = 0; b < batch; ++b) {
    dm_plan_blocks(n, gates + gate_begin[b], gate_count[b], plan, DmPlanOpts{kr && kr->n2 > 0, rot2});
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
  if (kr && kr->any()) dm_channel_tables(p1, p2, kr, T.dep);
  else dm_depol_tables(p1, p2, T.dep);
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
