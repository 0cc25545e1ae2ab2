// vqe_dm_grad.h - adjoint gradient of the batched exact channel mode (vqe_set_dm_grad on top of vqe_set_dm_batched,
// DESIGN 4.13).
//
// For one circuit rho_l = S_l rho_{l-1} over its L blocks and E = Re <Lambda_L, rho_L> with Lambda_L = conj(h), h the
// Hamiltonian as k_dm_energy_b sums it.  With Lambda_{l-1} = S_l^+ Lambda_l
//   dE/dtheta = Re sum_{r,c} (dS_l/dtheta)[r][c] M_l[r][c],   M_l[r][c] = sum over groups of conj(Lambda_l[g, r]) rho_{l-1}[g, c]
// where a group is the 16 entries of rho that one window position of block l ties together.  One lock-step evaluation of
// the resident batch (vqe_api.hip: dm_grad_eval) is
//   k_dm_build, k_dmg_adjoint     S of every block (vqe_dm_batch.h) and S^+ as a second table
//   per chunk of R resident circuits (buffers: Lambda [R], rho [level][R], level-major so that the kernels of
//   vqe_dm_batch.h see the slots of one level side by side):
//     k_dm_init_b                 rho_0
//     k_dmg_forward x L           rho_{l+1} = S rho_l OUT of place, k_dm_block_b's MFMA scheme; a circuit with fewer levels
//                                 copies, so rho_L of the chunk's last level is every circuit's final state and rho_{l-1}
//                                 is valid at each of its own levels.  Nothing is ever undone: the channels are singular
//                                 at p1 = 3/4 and p2 = 15/16.
//     k_dm_energy_b, k_dm_sum_b   E into fout[b]: the kernels and the bits of an energy run
//     k_dmg_lambda_zero / _set    Lambda_L = conj(h)
//     per level L .. 1:
//       k_dmg_macc                partial sums of M_l on v_mfma_f64_16x16x4_f64, K = groups; a lane loads the A / B
//                                 operand layout directly (entry = lane & 15 of group 4 j + (lane >> 4)), no LDS
//       k_dmg_msum                the partials in index order -> M of the block
//       k_dm_block_b              Lambda <- S^+ Lambda in place (the energy sweep's kernel on the second table)
//   k_dmg_contract                one workgroup per rotation member: dS (dm_build.h: the chain with the generator behind
//                                 the member) contracted with M of its block
//   k_dmg_scatter                 per circuit: the gradient zeroed, the members' values added in list order
// The split of a level's groups into partial sums is a function of n alone (dm_host.h: dm_grad_tiles_per_partial), so a
// circuit's gradient has the same bits whatever the batch, its position and R.  No atomics; every kernel takes `active`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vqe_dm_batch.h"

namespace vqe {

// S^+ of every block: Sd[c][r] = conj(S[r][c]).  One workgroup per block.
__global__ void __launch_bounds__(256) k_dmg_adjoint(DmBatchDev T, double* __restrict__ Sd, const int32_t* __restrict__ active) {
  const int k = blockIdx.x, t = threadIdx.x, r = t >> 4, c = t & 15;
  if (active && !active[T.blk_circ[k]]) return;
  const double* S = T.S + (size_t)k * 512;
  Sd[(size_t)k * 512 + c * 16 + r] = S[t];
  Sd[(size_t)k * 512 + 256 + c * 16 + r] = -S[256 + t];
}

// Level `level` of the chunk, out of place: dst slot = S src slot for circuit c0 + blockIdx.y, a plain copy where the
// circuit has no such level.  The sweep is k_dm_block_b's.
__global__ void __launch_bounds__(256) k_dmg_forward(const double2* __restrict__ src, double2* __restrict__ dst, DmBatchDev T, int n,
                                                     uint32_t n_groups, int level, int c0, const int32_t* __restrict__ active) {
  const int b = c0 + (int)blockIdx.y;
  if (active && !active[b]) return;
  const double2* __restrict__ in = src + ((size_t)blockIdx.y << (2 * n));
  double2* __restrict__ out = dst + ((size_t)blockIdx.y << (2 * n));
  const int k0 = T.blk_begin[b];
  if (level >= T.blk_begin[b + 1] - k0) {
    const size_t total = (size_t)1 << (2 * n);
    for (size_t f = (size_t)blockIdx.x * 256 + threadIdx.x; f < total; f += (size_t)gridDim.x * 256) out[f] = in[f];
    return;
  }
  const int k = k0 + level;
  const int wa = T.blk_win[6 * k], wb = T.blk_win[6 * k + 1];
  int hole[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) hole[i] = T.blk_win[6 * k + 2 + i];
  const double* __restrict__ S = T.S + (size_t)k * 512;
  const int lane = threadIdx.x & 63, q = lane >> 4, col = lane & 15;
  double sr[4], si[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sr[c] = S[col * 16 + 4 * c + q];
    si[c] = S[256 + col * 16 + 4 * c + q];
  }
  uint32_t eoff[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t e = (uint32_t)(q + 4 * c);
    eoff[c] = ((e & 1u) << wa) | (((e >> 1) & 1u) << wb) | (((e >> 2) & 1u) << (wa + n)) | (((e >> 3) & 1u) << (wb + n));
  }
  const uint32_t n_tiles = (n_groups + 15u) >> 4;
  const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, n_waves = gridDim.x * 4u;
  for (uint32_t t = wave; t < n_tiles; t += n_waves) {
    const uint32_t g = t * 16u + (uint32_t)col;
    const bool live = g < n_groups;
    uint32_t idx = live ? g : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int hb = hole[i];
      idx = ((idx >> hb) << (hb + 1)) | (idx & ((1u << hb) - 1u));
    }
    double2 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = live ? in[idx | eoff[c]] : make_double2(0.0, 0.0);
    dm_d4 accr = {0.0, 0.0, 0.0, 0.0}, acci = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      accr = __builtin_amdgcn_mfma_f64_16x16x4f64(sr[c], v[c].x, accr, 0, 0, 0);
      acci = __builtin_amdgcn_mfma_f64_16x16x4f64(si[c], v[c].x, acci, 0, 0, 0);
      accr = __builtin_amdgcn_mfma_f64_16x16x4f64(-si[c], v[c].y, accr, 0, 0, 0);
      acci = __builtin_amdgcn_mfma_f64_16x16x4f64(sr[c], v[c].y, acci, 0, 0, 0);
    }
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[idx | eoff[r]] = make_double2(accr[r], acci[r]);
    }
  }
}

// Lambda of the chunk's circuits to zero ...
__global__ void __launch_bounds__(256) k_dmg_lambda_zero(double2* __restrict__ lam, int n, int c0, const int32_t* __restrict__ active) {
  if (active && !active[c0 + (int)blockIdx.y]) return;
  const size_t total = (size_t)1 << (2 * n);
  double2* __restrict__ my = lam + (size_t)blockIdx.y * total;
  for (size_t f = (size_t)blockIdx.x * 256 + threadIdx.x; f < total; f += (size_t)gridDim.x * 256) my[f] = make_double2(0.0, 0.0);
}

// ... and conj(h) scattered into it: thread i, group g writes entry i | (i ^ x_g) << n, the one k_dm_energy_b reads with
// the same sum of signed coefficients.  Groups have distinct X masks, so no two writes meet.
__global__ void __launch_bounds__(256) k_dmg_lambda_set(double2* __restrict__ lam, int n, int n_groups, const uint32_t* __restrict__ gx,
                                                        const int32_t* __restrict__ term_off, const uint32_t* __restrict__ term_z,
                                                        const double* __restrict__ cr, const double* __restrict__ ci, int c0,
                                                        const int32_t* __restrict__ active) {
  if (active && !active[c0 + (int)blockIdx.y]) return;
  double2* __restrict__ my = lam + ((size_t)blockIdx.y << (2 * n));
  const uint32_t dim = 1u << n, i = blockIdx.x * 256u + threadIdx.x;
  if (i >= dim) return;
  for (int g = 0; g < n_groups; ++g) {
    const uint32_t x = gx[g];
    double dr = 0.0, di = 0.0;
    for (int k = term_off[g]; k < term_off[g + 1]; ++k) {
      const bool neg = __popc(i & term_z[k]) & 1;
      dr += neg ? -cr[k] : cr[k];
      di += neg ? -ci[k] : ci[k];
    }
    my[(size_t)i | ((size_t)(i ^ x) << n)] = make_double2(dr, -di);
  }
}

// Partial sums of M of level `level` (block k0 + level) for circuit c0 + blockIdx.y: wave w of the grid's x extent owns
// partial w = the tiles [w tpp, (w + 1) tpp) of 16 groups, in ascending order.  Per tile four MFMA steps of K = 4 groups:
// lane (q = lane >> 4, e = lane & 15) loads entry e of group 16 t + 4 j + q from Lambda (A[i = e][k = q], conjugated) and
// from rho (B[k = q][n = e]).  D: lane (q, e), register r = M[q + 4 r][e].  part: [slot][partial][2][16][16].
__global__ void __launch_bounds__(256) k_dmg_macc(const double2* __restrict__ rho, const double2* __restrict__ lam, DmBatchDev T, int n,
                                                  uint32_t n_groups, uint32_t tpp, uint32_t n_part, int level, int c0,
                                                  const int32_t* __restrict__ active, double* __restrict__ part) {
  const int b = c0 + (int)blockIdx.y;
  if (active && !active[b]) return;
  const int k0 = T.blk_begin[b];
  if (level >= T.blk_begin[b + 1] - k0) return;
  const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6;
  if (w >= n_part) return;
  const int k = k0 + level;
  const int wa = T.blk_win[6 * k], wb = T.blk_win[6 * k + 1];
  int hole[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) hole[i] = T.blk_win[6 * k + 2 + i];
  const double2* __restrict__ R = rho + ((size_t)blockIdx.y << (2 * n));
  const double2* __restrict__ L = lam + ((size_t)blockIdx.y << (2 * n));
  const int lane = threadIdx.x & 63, q = lane >> 4, e = lane & 15;
  const uint32_t eoff = (((uint32_t)e & 1u) << wa) | ((((uint32_t)e >> 1) & 1u) << wb) | ((((uint32_t)e >> 2) & 1u) << (wa + n)) |
                        ((((uint32_t)e >> 3) & 1u) << (wb + n));
  const uint32_t n_tiles = (n_groups + 15u) >> 4;
  const uint32_t t1 = (w + 1u) * tpp < n_tiles ? (w + 1u) * tpp : n_tiles;
  dm_d4 accr = {0.0, 0.0, 0.0, 0.0}, acci = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t t = w * tpp; t < t1; ++t) {
    double2 lv[4], rv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t g = t * 16u + 4u * (uint32_t)j + (uint32_t)q;
      const bool live = g < n_groups;
      uint32_t idx = live ? g : 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int hb = hole[i];
        idx = ((idx >> hb) << (hb + 1)) | (idx & ((1u << hb) - 1u));
      }
      lv[j] = live ? L[idx | eoff] : make_double2(0.0, 0.0);
      rv[j] = live ? R[idx | eoff] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {      // conj(l) r = (lx rx + ly ry) + i (lx ry - ly rx)
      accr = __builtin_amdgcn_mfma_f64_16x16x4f64(lv[j].x, rv[j].x, accr, 0, 0, 0);
      acci = __builtin_amdgcn_mfma_f64_16x16x4f64(lv[j].x, rv[j].y, acci, 0, 0, 0);
      accr = __builtin_amdgcn_mfma_f64_16x16x4f64(lv[j].y, rv[j].y, accr, 0, 0, 0);
      acci = __builtin_amdgcn_mfma_f64_16x16x4f64(-lv[j].y, rv[j].x, acci, 0, 0, 0);
    }
  }
  double* __restrict__ P = part + ((size_t)blockIdx.y * n_part + w) * 512;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    P[(q + 4 * r) * 16 + e] = accr[r];
    P[256 + (q + 4 * r) * 16 + e] = acci[r];
  }
}

// M of block k0 + level of circuit c0 + blockIdx.x: thread t sums word t of the partials in index order.  M: [block][2][16][16].
__global__ void __launch_bounds__(512) k_dmg_msum(const double* __restrict__ part, DmBatchDev T, uint32_t n_part, int level, int c0,
                                                  const int32_t* __restrict__ active, double* __restrict__ M) {
  const int b = c0 + (int)blockIdx.x;
  if (active && !active[b]) return;
  const int k0 = T.blk_begin[b];
  if (level >= T.blk_begin[b + 1] - k0) return;
  const double* __restrict__ P = part + (size_t)blockIdx.x * n_part * 512 + threadIdx.x;
  double sum = 0.0;
  for (uint32_t p = 0; p < n_part; ++p) sum += P[(size_t)p * 512];
  M[(size_t)(k0 + level) * 512 + threadIdx.x] = sum;
}

// One workgroup per member m of the batch's plan; a rotation member's workgroup builds dS of its block - k_dm_build's
// chain with the generator behind member m (dm_build.h) - and writes val[m] = Re sum dS[r][c] M[r][c], summed over the
// 256 entries in a fixed order.  mem_blk[m]: the block of member m.
__global__ void __launch_bounds__(256) k_dmg_contract(DmBatchDev T, const int32_t* __restrict__ mem_blk, const double* __restrict__ theta,
                                                      const int64_t* __restrict__ par_begin, const int32_t* __restrict__ active,
                                                      const double* __restrict__ M, double* __restrict__ val) {
  __shared__ double buf[2][2][256];
  __shared__ double red[4];
  const int which = blockIdx.x, wkind = T.mem[3 * which];
  if (!gate_is_rot(wkind)) return;
  const int k = mem_blk[which], b = T.blk_circ[k];
  if (active && !active[b]) return;
  const int t = threadIdx.x, r = t >> 4, c = t & 15;
  const double* th = theta + par_begin[b];
  int cur = 0;
  buf[0][0][t] = r == c ? 1.0 : 0.0;
  buf[0][1][t] = 0.0;
  __syncthreads();
  for (int m = T.mem_begin[k]; m < T.mem_begin[k + 1]; ++m) {
    const int kind = T.mem[3 * m], pos = T.mem[3 * m + 1], pidx = T.mem[3 * m + 2];
    double cs = 1.0, sn = 0.0;
    if (gate_is_rot(kind)) sincos(0.5 * th[pidx], &sn, &cs);
    double vr, vi;
    dm_build_entry(kind, pos, cs, sn, T.dep, buf[cur][0], buf[cur][1], r, c, vr, vi);
    buf[cur ^ 1][0][t] = vr;
    buf[cur ^ 1][1][t] = vi;
    cur ^= 1;
    __syncthreads();
    if (m == which) {
      dm_generator_apply_entry(kind, pos, buf[cur][0], buf[cur][1], r, c, vr, vi);
      buf[cur ^ 1][0][t] = vr;
      buf[cur ^ 1][1][t] = vi;
      cur ^= 1;
      __syncthreads();
    }
  }
  const double* Mk = M + (size_t)k * 512;
  double acc = buf[cur][0][t] * Mk[t] - buf[cur][1][t] * Mk[256 + t];
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) val[which] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per circuit: grad[par_begin[b] .. + par_count[b]) = 0, then the values of its rotation members added to
// their parameters in list order (blocks in sweep order, members in block order) by one thread.  A parameter no gate
// uses stays exactly 0.0.
__global__ void __launch_bounds__(64) k_dmg_scatter(DmBatchDev T, const int64_t* __restrict__ par_begin, const int32_t* __restrict__ par_count,
                                                    const int32_t* __restrict__ active, const double* __restrict__ val,
                                                    double* __restrict__ grad) {
  const int b = blockIdx.x;
  if (active && !active[b]) return;
  double* g = grad + par_begin[b];
  for (int j = threadIdx.x; j < par_count[b]; j += 64) g[j] = 0.0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int m = T.mem_begin[T.blk_begin[b]]; m < T.mem_begin[T.blk_begin[b + 1]]; ++m) {
    const int kind = T.mem[3 * m];
    if (gate_is_rot(kind)) g[T.mem[3 * m + 2]] += val[m];
  }
}

// active[b] of the device L-BFGS records (k_sl_step keeps its running flag inside StreamLbfgsRec): the flags as the array
// the evaluation kernels take.  flag: the address of rec[0].active, stride: sizeof(StreamLbfgsRec) / 4.
__global__ void __launch_bounds__(64) k_dmg_active(const int32_t* __restrict__ flag, int stride, int batch, int32_t* __restrict__ active) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < batch) active[b] = flag[(size_t)b * stride];
}

}  // namespace vqe
