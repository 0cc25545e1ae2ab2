// vqe_grad_body.h - steps 1 (after compile_ops) to 4 of the adjoint evaluation (vqe_grad.h), as text.
//
// Included in the circuit loop of k_lds_energy_grad and in the device function adjoint_eval (which k_lds_minimize_lbfgs
// calls once per trial point).  It is text and not a call because k_lds_energy_grad<13,true> sits at its register limit:
// with the body behind a function boundary, however spelled, the register allocator spilled 24 VGPRs more;
// expanded in place the kernel compiles to what it compiled to before the body was shared.
// Expects in scope: N, NT, NW, DIM, NA, NP, BACKWARD, NOISY (compile-time); A (BatchArgs), GH (GradHam), L (Lds, ops compiled),
// lam, gacc, theta, P, tid, wave; the macro ADJOINT_GRAD_DST(j), the lvalue entry j of the gradient goes to.
// NOISY (one realisation of a Pauli-noise trajectory): L.ops come from a `slots` compile and carry the patch
// of this realisation (patch_noise<N, true>); also in scope nz_t, nz_T - the realisation and their number: entry j of the
// gradient is overwritten at nz_t = 0, added to afterwards (by the same thread every time) and divided by nz_T at the
// last one.  gacc has one row per op WITH a parameter, numbered from the last op backwards.  Every NOISY statement sits
// behind `if constexpr`: the noiseless instances compile to what they compiled to without them.
// Leaves `e` (the energy, in every thread) in scope.  Ends with every read of the LDS state done except those of
// step 4 (ops, gacc).
    // ---- 1. forward pass in the physical frame
    const uint32_t coff = (uint32_t)L.meta[1];
    const int permuted = NOISY ? (L.meta[6] | (int)(coff != 0u)) : L.meta[6];   // (X errors move c: the frame of this realisation)
    load_init<N>(L, A.init);
    if (tid == 0) L.meta[3] = 0;                  // no final gather: run_ops leaves psi physical
    __syncthreads();
    run_ops<N, NOISY>(L, theta, P);
    // ---- gather into logical order and 2. lambda = H psi, E = Re <psi|lambda> (shared with vqe_qjump.h)
#include "vqe_grad_energy.h"
    if constexpr (BACKWARD) {                     // (not for the energy alone: the last evaluation of an environment step)
    // back to the physical frame: psi[phys(i)] = psi_logical[i], the same for lambda
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const uint32_t i = tid + (uint32_t)k * NT;
      if (DIM >= NT || i < DIM) {
        const uint32_t p = permuted ? phys(i) : i;
        L.psi[p] = own[k];
        lam[p] = acc[k];
      }
    }
    __syncthreads();
    // ---- 3. backward pass
    const int nops = L.meta[0];
    int grow = 0;                                 // NOISY: row of gacc the next op with a parameter writes
    for (int o = nops - 1; o >= 0; --o) {
      const Op op = L.ops[o];
      const int kind = op.kind & 0xff;
      const int inv = (op.kind >> 8) & 1;
      if constexpr (NOISY) {
        if (kind == OP_NOP) continue;             // inactive slot: no work, no row, no barrier
        if (kind == OP_PZ) {
          // an active Z slot: its +-1 diagonal (its own inverse) on psi and lambda; the generators in front of it do not
          // commute with it, so it cannot be left out
#pragma unroll
          for (int k = 0; k < NA; ++k) {
            const uint32_t p = tid + (uint32_t)k * NT;
            if ((DIM >= NT || p < DIM) && (parity32(p & op.zm) ^ inv)) {
              const double2 a = L.psi[p], l = lam[p];
              L.psi[p] = make_double2(-a.x, -a.y);
              lam[p] = make_double2(-l.x, -l.y);
            }
          }
          __syncthreads();
          continue;
        }
      }
      const double2 cs = L.cs[op.pidx];           // (slots have pidx = -1: they never get here)
      const double c = cs.x, s = cs.y;
      double gp = 0.0;
      if (op_is_pair(kind)) {
        const int hb = 31 - __clz((int)op.xm);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const uint32_t q = tid + (uint32_t)k * NT;
          if (DIM / 2 >= NT || q < DIM / 2) {
            const uint32_t p0 = insert0(q, hb), p1 = p0 ^ op.xm;
            const double2 a0 = L.psi[p0], a1 = L.psi[p1];
            const double2 l0 = lam[p0], l1 = lam[p1];
            if (kind == OP_RX) {
              // K = iX: (K psi)[p0] = i a1, (K psi)[p1] = i a0
              gp += l0.x * -a1.y + l0.y * a1.x + l1.x * -a0.y + l1.y * a0.x;
              // U^-1 = c I - s iX
              L.psi[p0] = make_double2(c * a0.x + s * a1.y, c * a0.y - s * a1.x);
              L.psi[p1] = make_double2(c * a1.x + s * a0.y, c * a1.y - s * a0.x);
              lam[p0] = make_double2(c * l0.x + s * l1.y, c * l0.y - s * l1.x);
              lam[p1] = make_double2(c * l1.x + s * l0.y, c * l1.y - s * l0.x);
            } else if (kind == OP_RYY) {
              const double sg = (parity32(p0 & op.zm) ^ inv) ? 1.0 : -1.0;
              // K = i sg X with one sign per pair: (K psi)[p0] = i sg a1, (K psi)[p1] = i sg a0
              gp += sg * (l0.x * -a1.y + l0.y * a1.x + l1.x * -a0.y + l1.y * a0.x);
              const double s0 = sg * s;
              L.psi[p0] = make_double2(c * a0.x + s0 * a1.y, c * a0.y - s0 * a1.x);
              L.psi[p1] = make_double2(c * a1.x + s0 * a0.y, c * a1.y - s0 * a0.x);
              lam[p0] = make_double2(c * l0.x + s0 * l1.y, c * l0.y - s0 * l1.x);
              lam[p1] = make_double2(c * l1.x + s0 * l0.y, c * l1.y - s0 * l0.x);
            } else {
              const double sg = (parity32(p0 & op.zm) ^ inv) ? -1.0 : 1.0;
              // K: (K psi)[p0] = sg a1, (K psi)[p1] = -sg a0
              gp += sg * (l0.x * a1.x + l0.y * a1.y - l1.x * a0.x - l1.y * a0.y);
              const double s0 = sg * s;
              L.psi[p0] = make_double2(c * a0.x - s0 * a1.x, c * a0.y - s0 * a1.y);
              L.psi[p1] = make_double2(c * a1.x + s0 * a0.x, c * a1.y + s0 * a0.y);
              lam[p0] = make_double2(c * l0.x - s0 * l1.x, c * l0.y - s0 * l1.y);
              lam[p1] = make_double2(c * l1.x + s0 * l0.x, c * l1.y + s0 * l0.y);
            }
          }
        }
      } else if (kind == OP_RZ) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
          const uint32_t p = tid + (uint32_t)k * NT;
          if (DIM >= NT || p < DIM) {
            const double sg = (parity32(p & op.zm) ^ inv) ? -1.0 : 1.0;
            const double2 a = L.psi[p], l = lam[p];
            // K = i sg: (K psi)[p] = sg (-a.y, a.x)
            gp += sg * (l.y * a.x - l.x * a.y);
            const double ss = sg * s;
            L.psi[p] = make_double2(c * a.x + ss * a.y, c * a.y - ss * a.x);
            lam[p] = make_double2(c * l.x + ss * l.y, c * l.y - ss * l.x);
          }
        }
      }
      gp = wave_sum(gp);
      if constexpr (NOISY) {
        if ((tid & 63u) == 0u) gacc[grow * NW + wave] = gp;
        ++grow;
      } else {
        if ((tid & 63u) == 0u) gacc[o * NW + wave] = gp;
      }
      __syncthreads();
    }
    // ---- 4. per-parameter sums (a parameter may be shared by several gates; an unused one gets 0)
    for (int j = (int)tid; j < P; j += NT) {
      double gsum = 0.0;
      if constexpr (NOISY) {
        int r = 0;
        for (int o = nops - 1; o >= 0; --o) {     // the order the rows were written in
          const int pj = L.ops[o].pidx;
          if (pj < 0) continue;
          if (pj == j) {
#pragma unroll
            for (int w = 0; w < NW; ++w) gsum += gacc[r * NW + w];
          }
          ++r;
        }
        if (nz_t > 0) gsum = ADJOINT_GRAD_DST(j) + gsum;
        if (nz_t == nz_T - 1) gsum = gsum / (double)nz_T;
      } else {
        for (int o = 0; o < nops; ++o) {
          if (L.ops[o].pidx != j) continue;
#pragma unroll
          for (int w = 0; w < NW; ++w) gsum += gacc[o * NW + w];
        }
      }
      ADJOINT_GRAD_DST(j) = gsum;
    }
    }  // BACKWARD
