// vqe_grad_energy.h - the end of step 1 and step 2 of the adjoint evaluation (vqe_grad_body.h), as text: the gather of
// the physical-frame state into logical order and E = Re <psi| H psi> on the GradHam tables.
//
// Included by vqe_grad_body.h (every adjoint kernel) and by the trajectory kernel of vqe_qjump.h, whose forward sweep is
// its own.  Text for the reason vqe_grad_body.h gives.
// Expects in scope: N, NT, NW, DIM, NA (compile-time); GH (GradHam), L (Lds: psi in the physical frame, xm), tid;
// permuted (the frame differs from the logical order) and coff (the offset c of the frame).
// Leaves in scope: own[] (this thread's amplitudes, logical order), acc[] (those of H psi), e (the energy, in every
// thread); L.psi holds the state in logical order.  Ends with a barrier.
    // physical index of logical index i: A^-1 (i ^ c)
    auto phys = [&](uint32_t i) {
      const uint32_t v = i ^ coff;
      uint32_t p = 0;
#pragma unroll
      for (int q = 0; q < N; ++q) p ^= ((v >> q) & 1u) ? L.xm[q] : 0u;
      return p;
    };
    double2 own[NA];
    if (permuted) {
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const uint32_t i = tid + (uint32_t)k * NT;
        if (DIM >= NT || i < DIM) own[k] = L.psi[phys(i)];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const uint32_t i = tid + (uint32_t)k * NT;
        if (DIM >= NT || i < DIM) L.psi[i] = own[k];
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const uint32_t i = tid + (uint32_t)k * NT;
        if (DIM >= NT || i < DIM) own[k] = L.psi[i];
      }
    }
    // ---- 2. lambda = H psi (logical frame), E = Re <psi|lambda>
    double2 acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = make_double2(0.0, 0.0);
    for (int g = 0; g < GH.n_groups; ++g) {
      const uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)GH.gx[g]);
      const double* t = GH.tab + GH.off[g];
      if (x == 0u) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
          const uint32_t i = tid + (uint32_t)k * NT;
          if (DIM >= NT || i < DIM) {
            const double d = t[i];
            acc[k].x += d * own[k].x;
            acc[k].y += d * own[k].y;
          }
        }
        continue;
      }
      const int hb = 31 - __clz((int)x);
      const bool cplx = __builtin_amdgcn_readfirstlane(GH.cplx[g]) != 0;
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const uint32_t i = tid + (uint32_t)k * NT;
        if (DIM >= NT || i < DIM) {
          const uint32_t j = i ^ x;
          const uint32_t up = (i >> hb) & 1u;            // 1: i is the p0 ^ x member of its pair
          const uint32_t i0 = up ? j : i;
          const uint32_t q = ((i0 >> (hb + 1)) << hb) | (i0 & ((1u << hb) - 1u));
          const double2 a = L.psi[j];
          if (cplx) {
            const double2 d = ((const double2*)t)[q];
            const double di = up ? d.y : -d.y;           // T for the p0 -> p0 ^ x direction, conj(T) for the other
            acc[k].x += d.x * a.x - di * a.y;
            acc[k].y += d.x * a.y + di * a.x;
          } else {
            const double d = t[q];
            acc[k].x += d * a.x;
            acc[k].y += d * a.y;
          }
        }
      }
    }
    double e_part = 0.0;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const uint32_t i = tid + (uint32_t)k * NT;
      if (DIM >= NT || i < DIM) e_part += own[k].x * acc[k].x + own[k].y * acc[k].y;
    }
    const double e = block_sum<NW>(e_part, L.red);   // (its barriers also end every read of psi above)
    __syncthreads();
