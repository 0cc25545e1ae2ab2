// vqe_dm_batch.h - the exact channel mode (vqe_dm.h) for a resident batch in lock-step (vqe_set_dm_batched).
//
// The serial path builds the superoperator blocks of ONE circuit on the host, uploads them and launches one sweep per
// block, for every trial point of every circuit.  Here the block structure is planned once per resident batch
// (dm_host.h: dm_plan_blocks / dm_flatten_plans - it does not depend on the angles) and an evaluation of the whole batch
// at the trial points in theta is
//   k_dm_build          one workgroup per (circuit, block): S from the member list and the angles (dm_build.h)
//   per chunk of R resident density matrices:
//     k_dm_init_b       rho_b = |psi0><psi0|                                  grid.y = circuit of the chunk
//     k_dm_block_b x L  level l: circuit b applies ITS l-th block (window bits and S from the tables); a circuit with
//                       fewer blocks leaves at once.  The MFMA scheme of k_dm_block, in place, no LDS.
//     k_dm_energy_b, k_dm_sum_b   per-workgroup partials, then a fixed-order sum per circuit into fout[b]
// all on one stream with nothing copied to the host.  Every kernel takes the `active` array of k_s_cobyla (NULL: all
// circuits): a circuit whose optimiser has finished costs an early exit per workgroup and its fout[b] is left alone.
// What a circuit computes depends on its own gates and angles only - not on the batch around it, its position or the
// chunk size - and no atomics are used: same bits wherever it sits.  Per-circuit base offsets are size_t (260 density
// matrices of 10 qubits are 4.06 GiB).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vqe_dm.h"
#include "dm_build.h"

namespace vqe {

struct DmBatchDev {      // device copy of DmBatchTables (dm_host.h) + the matrices k_dm_build writes
  const int32_t* blk_begin;
  const int32_t* blk_circ;
  const int32_t* blk_win;
  const int32_t* mem_begin;
  const int32_t* mem;
  const double* dep;
  double* S;             // [block][2][16][16]
};

// One workgroup per block of the batch, thread t owns entry (t >> 4, t & 15); S double-buffered in LDS (2 x 4 KiB).
__global__ void __launch_bounds__(256) k_dm_build(DmBatchDev T, const double* __restrict__ theta, const int64_t* __restrict__ par_begin,
                                                  const int32_t* __restrict__ active) {
  __shared__ double buf[2][2][256];
  const int k = blockIdx.x, b = T.blk_circ[k];
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
  }
  double* S = T.S + (size_t)k * 512;
  S[t] = buf[cur][0][t];
  S[256 + t] = buf[cur][1][t];
}

// rho of the chunk's circuits c0 + blockIdx.y: slot blockIdx.y of the resident buffer
__global__ void __launch_bounds__(256) k_dm_init_b(double2* __restrict__ rho, const double2* __restrict__ psi0, int n, int c0,
                                                   const int32_t* __restrict__ active) {
  if (active && !active[c0 + (int)blockIdx.y]) return;
  const size_t total = (size_t)1 << (2 * n);
  double2* __restrict__ my = rho + (size_t)blockIdx.y * total;
  const uint32_t mask = (1u << n) - 1u;
  for (size_t f = (size_t)blockIdx.x * 256 + threadIdx.x; f < total; f += (size_t)gridDim.x * 256) {
    const double2 k = psi0[(uint32_t)f & mask], bq = psi0[(uint32_t)(f >> n)];
    my[f] = make_double2(k.x * bq.x + k.y * bq.y, k.y * bq.x - k.x * bq.y);      // psi_i conj(psi_j)
  }
}

// Level `level` of the chunk: circuit c0 + blockIdx.y applies its level-th block.  k_dm_block's scheme: a lane loads the
// four entries e = q + 4 c of its group that the D layout of v_mfma_f64_16x16x4_f64 hands back to it.
__global__ void __launch_bounds__(256) k_dm_block_b(double2* __restrict__ rho, DmBatchDev T, int n, uint32_t n_groups, int level, int c0,
                                                    const int32_t* __restrict__ active) {
  const int b = c0 + (int)blockIdx.y;
  if (active && !active[b]) return;
  const int k0 = T.blk_begin[b];
  if (level >= T.blk_begin[b + 1] - k0) return;
  const int k = k0 + level;
  const int wa = T.blk_win[6 * k], wb = T.blk_win[6 * k + 1];
  int hole[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) hole[i] = T.blk_win[6 * k + 2 + i];
  const double* __restrict__ S = T.S + (size_t)k * 512;
  double2* __restrict__ my = rho + ((size_t)blockIdx.y << (2 * n));
  const int lane = threadIdx.x & 63, q = lane >> 4, col = lane & 15;
  // A operands: S[m = lane & 15][k = 4 c + q] (A[i][k]: lane = i + 16 k)
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
    const bool live = g < n_groups;      // n = 2, 3: fewer than 16 groups
    uint32_t idx = live ? g : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {      // a zero at every window bit, lowest first
      const int hb = hole[i];
      idx = ((idx >> hb) << (hb + 1)) | (idx & ((1u << hb) - 1u));
    }
    double2 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = live ? my[idx | eoff[c]] : make_double2(0.0, 0.0);
    dm_d4 accr = {0.0, 0.0, 0.0, 0.0}, acci = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {      // B[k][n]: lane = n + 16 k holds entry k = 4 c + q of group n
      accr = __builtin_amdgcn_mfma_f64_16x16x4f64(sr[c], v[c].x, accr, 0, 0, 0);
      acci = __builtin_amdgcn_mfma_f64_16x16x4f64(si[c], v[c].x, acci, 0, 0, 0);
      accr = __builtin_amdgcn_mfma_f64_16x16x4f64(-si[c], v[c].y, accr, 0, 0, 0);
      acci = __builtin_amdgcn_mfma_f64_16x16x4f64(sr[c], v[c].y, acci, 0, 0, 0);
    }
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; ++r) my[idx | eoff[r]] = make_double2(accr[r], acci[r]);   // D row = q + 4 reg
    }
  }
}

// k_dm_energy per circuit of the chunk: partial[slot][workgroup]
__global__ void __launch_bounds__(256) k_dm_energy_b(const double2* __restrict__ rho, int n, int n_groups,
                                                    const uint32_t* __restrict__ gx, const int32_t* __restrict__ term_off,
                                                    const uint32_t* __restrict__ term_z, const double* __restrict__ cr,
                                                    const double* __restrict__ ci, double* __restrict__ partial, int c0,
                                                    const int32_t* __restrict__ active) {
  __shared__ double red[4];
  if (active && !active[c0 + (int)blockIdx.y]) return;
  const double2* __restrict__ my = rho + ((size_t)blockIdx.y << (2 * n));
  const uint32_t dim = 1u << n, i = blockIdx.x * 256u + threadIdx.x;
  double acc = 0.0;
  if (i < dim) {
    for (int g = 0; g < n_groups; ++g) {
      const uint32_t x = gx[g];
      const double2 r = my[(size_t)i | ((size_t)(i ^ x) << n)];
      double dr = 0.0, di = 0.0;
      for (int k = term_off[g]; k < term_off[g + 1]; ++k) {
        const bool neg = __popc(i & term_z[k]) & 1;
        dr += neg ? -cr[k] : cr[k];
        di += neg ? -ci[k] : ci[k];
      }
      acc += r.x * dr - r.y * di;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one thread per circuit of the chunk: the partials in index order
__global__ void __launch_bounds__(64) k_dm_sum_b(const double* __restrict__ partial, int n_blocks, int count, int c0,
                                                const int32_t* __restrict__ active, double* __restrict__ fout) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= count) return;
  if (active && !active[c0 + s]) return;
  double sum = 0.0;
  for (int j = 0; j < n_blocks; ++j) sum += partial[(size_t)s * n_blocks + j];
  fout[c0 + s] = sum;
}

}  // namespace vqe
