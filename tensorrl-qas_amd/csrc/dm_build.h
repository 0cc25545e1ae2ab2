// dm_build.h - the per-block builder of the batched exact channel mode: the 16 x 16 superoperator of one block from its
// member list (dm_host.h: DmBatchTables) and the circuit's angles.  One function, compiled for the device by k_dm_build
// (vqe_dm_batch.h) and for the host by tests/cpp/dm_plan_check.cpp, which holds it against dm_fill_blocks.  Below it the
// derivative chain of the adjoint gradient (vqe_dm_grad.h): the same product with a rotation's generator behind it.
//
// Fixed order: S = identity; for the members in list order S <- G S, every entry of the product summed over the inner
// index ascending.  The unit of work is ONE ENTRY (r, c) of one product, which is what a thread of k_dm_build owns; the
// caller keeps S double-buffered and runs the entries of a member in any order (or side by side).
// Plain C++ without the standard library: no std::complex on the device.
#pragma once
#include "vqe_geo.h"

namespace vqe {

// entry (r, k) of one member's superoperator: G[(i, j), (i', j')] = U[i][i'] conj(U[j][j']), r = i + 4 j, k = i' + 4 j'
// (i = ket bits (a, b), j = bra bits).  cs / sn: cos / sin of half the member's angle (rotations only); dep: the
// channel tables of DmBatchTables (a two-qubit channel reads slice 2 + pos; pos is 0 unless a two-qubit Kraus set is
// installed).

// entry [x][y] of P (x) P on the window for kind = G_RXX / G_RYY / G_RZZ: real and symmetric for all three
VQE_HD inline double dm_pauli2_entry(int kind, int x, int y) {
  const double even = ((x ^ (x >> 1)) & 1) ? -1.0 : 1.0;      // +1 on |00>, |11>
  if (kind == G_RZZ) return x == y ? even : 0.0;
  if (x != (y ^ 3)) return 0.0;
  return kind == G_RXX ? 1.0 : -even;                          // Y (x) Y: -1 between |00> and |11>, +1 between |01> and |10>
}

VQE_HD inline void dm_member_entry(int kind, int pos, double cs, double sn, const double* dep, int r, int k, double& gr, double& gi) {
  if (kind == G_DEPOL1 || kind == G_DEPOL2) {
    const double* t = dep + (kind == G_DEPOL2 ? 2 + pos : pos) * 512;
    gr = t[r * 16 + k];
    gi = t[256 + r * 16 + k];
    return;
  }
  const int i = r & 3, j = r >> 2, ip = k & 3, jp = k >> 2;
  if (gate_is_rot2(kind)) {      // U = cs I + i sn P (x) P: U[x][y] = cs [x == y] + i sn PP[x][y]
    const double ur = i == ip ? cs : 0.0, ui_ = sn * dm_pauli2_entry(kind, i, ip);
    const double vr = j == jp ? cs : 0.0, vi = sn * dm_pauli2_entry(kind, j, jp);
    gr = ur * vr + ui_ * vi;      // U[i][ip] conj(U[j][jp])
    gi = ui_ * vr - ur * vi;
    return;
  }
  if (kind == G_CNOT) {      // pos: the control's window position
    const int pt = pos ^ 1;
    const bool ui = i == (ip ^ (((ip >> pos) & 1) << pt)), uj = j == (jp ^ (((jp >> pos) & 1) << pt));
    gr = (ui && uj) ? 1.0 : 0.0;
    gi = 0.0;
    return;
  }
  // a rotation on window position pos: U[x][y] = R[x_pos][y_pos] where the other bit agrees, else 0
  const int other = pos ^ 1;
  if (((i >> other) & 1) != ((ip >> other) & 1) || ((j >> other) & 1) != ((jp >> other) & 1)) { gr = 0.0; gi = 0.0; return; }
  double ur, ui_, vr, vi;      // U[i][ip], U[j][jp]
  const int a0 = (i >> pos) & 1, a1 = (ip >> pos) & 1, b0 = (j >> pos) & 1, b1 = (jp >> pos) & 1;
  if (kind == G_RX) {
    ur = a0 == a1 ? cs : 0.0; ui_ = a0 == a1 ? 0.0 : sn;
    vr = b0 == b1 ? cs : 0.0; vi = b0 == b1 ? 0.0 : sn;
  } else if (kind == G_RY) {
    ur = a0 == a1 ? cs : (a0 == 0 ? sn : -sn); ui_ = 0.0;
    vr = b0 == b1 ? cs : (b0 == 0 ? sn : -sn); vi = 0.0;
  } else {      // G_RZ
    ur = a0 == a1 ? cs : 0.0; ui_ = a0 != a1 ? 0.0 : (a0 == 0 ? sn : -sn);
    vr = b0 == b1 ? cs : 0.0; vi = b0 != b1 ? 0.0 : (b0 == 0 ? sn : -sn);
  }
  gr = ur * vr + ui_ * vi;      // U[i][ip] conj(U[j][jp])
  gi = ui_ * vr - ur * vi;
}

// entry (r, c) of G S for one member: sum over k ascending of G[r][k] S[k][c].  sr / si: S, row-major [16][16].
VQE_HD inline void dm_build_entry(int kind, int pos, double cs, double sn, const double* dep, const double* sr, const double* si,
                                  int r, int c, double& outr, double& outi) {
  double vr = 0.0, vi = 0.0;
  for (int k = 0; k < 16; ++k) {
    double gr, gi;
    dm_member_entry(kind, pos, cs, sn, dep, r, k, gr, gi);
    const double xr = sr[k * 16 + c], xi = si[k * 16 + c];
    vr += gr * xr - gi * xi;
    vi += gr * xi + gi * xr;
  }
  outr = vr;
  outi = vi;
}

// ---- the derivative chain (vqe_dm_grad.h) -------------------------------------------------------------
// A rotation member is rho -> U rho U^+ with U = exp(+i theta/2 P), so d/dtheta of it is D G with the fixed generator
// D rho = (i/2) (P rho - rho P):  D[(i, j), (i', j')] = (i/2) (P[i][i'] [j == j'] - [i == i'] P[j'][j]), P acting on
// window position pos.  dS/dtheta of a block is its member list with D inserted behind the member.  A two-qubit
// rotation has P (x) P on the whole window in P's place (real and symmetric: D is purely imaginary).
VQE_HD inline void dm_generator_entry(int kind, int pos, int r, int k, double& gr, double& gi) {
  const int i = r & 3, j = r >> 2, ip = k & 3, jp = k >> 2, other = pos ^ 1;
  gr = 0.0;
  gi = 0.0;
  if (gate_is_rot2(kind)) {
    gi = 0.5 * ((j == jp ? dm_pauli2_entry(kind, i, ip) : 0.0) - (i == ip ? dm_pauli2_entry(kind, jp, j) : 0.0));
    return;
  }
  for (int side = 0; side < 2; ++side) {      // 0: (i/2) P on the ket index, 1: -(i/2) P^T on the bra index
    const int x = side ? jp : i, y = side ? j : ip;      // the entry P[x][y] that is wanted
    if ((side ? i != ip : j != jp) || ((x >> other) & 1) != ((y >> other) & 1)) continue;
    const int a = (x >> pos) & 1, b = (y >> pos) & 1;
    double pr = 0.0, pi = 0.0;
    if (kind == G_RX) pr = a != b ? 1.0 : 0.0;
    else if (kind == G_RY) pi = a == b ? 0.0 : (a == 0 ? -1.0 : 1.0);
    else pr = a != b ? 0.0 : (a == 0 ? 1.0 : -1.0);
    const double s = side ? -0.5 : 0.5;      // (+-i/2) (pr + i pi)
    gr += -s * pi;
    gi += s * pr;
  }
}

// entry (r, c) of D S: dm_build_entry with the generator in the member's place
VQE_HD inline void dm_generator_apply_entry(int kind, int pos, const double* sr, const double* si, int r, int c, double& outr, double& outi) {
  double vr = 0.0, vi = 0.0;
  for (int k = 0; k < 16; ++k) {
    double gr, gi;
    dm_generator_entry(kind, pos, r, k, gr, gi);
    const double xr = sr[k * 16 + c], xi = si[k * 16 + c];
    vr += gr * xr - gi * xi;
    vi += gr * xi + gi * xr;
  }
  outr = vr;
  outi = vi;
}

// dS/dtheta of one block for its rotation member `which` (index into the block's member list), into (outr, outi)
// [16][16] row-major: the chain of k_dm_build with D behind that member.  mem: the block's members (3 ints each),
// cs / sn: cos / sin of half the angle of every member (1, 0 where it is no rotation).  tr / ti: 2 x 256 doubles of
// work space.  The serial form of what a workgroup of k_dmg_contract runs entry by entry; tests/cpp/dm_grad_check.cpp
// holds it against the exact shift of dm_fill_blocks.
VQE_HD inline void dm_block_derivative(const int32_t* mem, int n_mem, int which, const double* cs, const double* sn, const double* dep,
                                       double* outr, double* outi, double* tr, double* ti) {
  double* cr = outr; double* ci = outi; double* nr = tr; double* ni = ti;
  for (int t = 0; t < 256; ++t) { cr[t] = (t >> 4) == (t & 15) ? 1.0 : 0.0; ci[t] = 0.0; }
  for (int m = 0; m < n_mem; ++m) {
    const int kind = mem[3 * m], pos = mem[3 * m + 1];
    for (int pass = 0; pass < (m == which ? 2 : 1); ++pass) {
      for (int t = 0; t < 256; ++t) {
        if (pass == 0) dm_build_entry(kind, pos, cs[m], sn[m], dep, cr, ci, t >> 4, t & 15, nr[t], ni[t]);
        else dm_generator_apply_entry(kind, pos, cr, ci, t >> 4, t & 15, nr[t], ni[t]);
      }
      double* s = cr; cr = nr; nr = s;
      s = ci; ci = ni; ni = s;
    }
  }
  if (cr != outr) for (int t = 0; t < 256; ++t) { outr[t] = cr[t]; outi[t] = ci[t]; }
}

}  // namespace vqe
