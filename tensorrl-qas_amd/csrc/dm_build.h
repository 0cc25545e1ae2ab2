// dm_build.h - the per-block builder of the batched exact channel mode: the 16 x 16 superoperator of one block from its
// member list (dm_host.h: DmBatchTables) and the circuit's angles.  One function, compiled for the device by k_dm_build
// (vqe_dm_batch.h) and for the host by tests/cpp/dm_plan_check.cpp, which holds it against dm_fill_blocks.
//
// Fixed order: S = identity; for the members in list order S <- G S, every entry of the product summed over the inner
// index ascending.  The unit of work is ONE ENTRY (r, c) of one product, which is what a thread of k_dm_build owns; the
// caller keeps S double-buffered and runs the entries of a member in any order (or side by side).
// Plain C++ without the standard library: no std::complex on the device.
#pragma once
#include "vqe_geo.h"

namespace vqe {

// entry (r, k) of one member's superoperator: G[(i, j), (i', j')] = U[i][i'] conj(U[j][j']), r = i + 4 j, k = i' + 4 j'
// (i = ket bits (a, b), j = bra bits).  cs / sn: cos / sin of half the member's angle (rotations only); dep: the three
// channel tables of DmBatchTables.
VQE_HD inline void dm_member_entry(int kind, int pos, double cs, double sn, const double* dep, int r, int k, double& gr, double& gi) {
  if (kind == G_DEPOL1 || kind == G_DEPOL2) {
    const double* t = dep + (kind == G_DEPOL2 ? 2 : pos) * 512;
    gr = t[r * 16 + k];
    gi = t[256 + r * 16 + k];
    return;
  }
  const int i = r & 3, j = r >> 2, ip = k & 3, jp = k >> 2;
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

}  // namespace vqe
