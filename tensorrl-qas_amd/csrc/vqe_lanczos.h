// vqe_lanczos.h - device Lanczos for the extreme eigenpair of the handle's Hamiltonian (vqe_lanczos).
//
// Lanczos with a stored basis, full reorthogonalisation (two passes of classical Gram-Schmidt against every stored
// vector) and explicit restart from the current Ritz vector when the basis is full.  Every vector is complex128[2^n] in
// global memory, the same path for every n.  The operator is the FULL Hamiltonian of the handle in the LOGICAL frame,
// grouped by X mask with explicit terms (z mask, Re and Im of c i^#Y), built from the handle's host copy into buffers of
// the solver's own (the tables of the energy kernels are in another frame at n <= 13 and hold only a shard).
//
// One Lanczos step j queues kernels only:
//   k_lz_apply  w = H v_j - beta_{j-1} v_{j-1} (gather form: a thread owns amplitudes, so no two threads write one entry;
//               the term tables are read wave-uniformly) and the block partials of alpha_j = Re <v_j|w>;
//   k_lz_axpy   w -= alpha_j v_j;
//   twice:      k_lz_proj (a block loads its slice of w once and loops over v_0 .. v_j, partials [k][block]),
//               k_lz_coef (c_k = the sum of row k), k_lz_sub (w -= sum_k c_k v_k, block partials of |w|^2);
//   k_lz_norm   beta_j = |w|, v_{j+1} = w / beta_j, alpha_j and beta_j into the device arrays the host looks at.
// No atomics: a kernel writes one partial per block, the consumer adds them in index order (lz_sum: staged in LDS,
// one thread adds them one after the other), so a run has the same bits every time and every block of a consumer holds
// the same value.  A negligible beta_j is a breakdown (an exact invariant subspace): k_lz_norm does
// not divide and sets a device flag on which every kernel queued behind it exits at once.  The host reads alpha, beta
// and the flag every check_every steps (lanczos_host.h: lz_decide) and never anything state-sized.
//
// Several eigenpairs with their multiplicities (vqe_lanczos_multi) are at the end of the file: the same
// step kernels driven by the LzMulti state machine, one stage per pair, and k_lz_rotate for the thick restart.
#pragma once
#include "vqe_device.h"
#include "vqe_devbuf.h"
#include "ham_layout.h"
#include "lanczos_host.h"

#include <string>
#include <vector>

namespace vqe {

constexpr int kLzThreads = 256;
constexpr int kLzApt = 4;                               // amplitudes of a chunk a thread owns
constexpr uint32_t kLzChunk = kLzThreads * kLzApt;      // amplitudes of a chunk; block b takes chunks b, b + grid, ..
constexpr int kLzMaxBlocks = 1024;                      // grid cap (one chunk per block up to 20 qubits)
constexpr int kLzProjTile = 32;                         // basis vectors between two barriers of k_lz_proj

struct LzHam {
  int n_groups;
  const uint32_t* gx;      // [n_groups] X mask
  const int32_t* toff;     // [n_groups + 1] terms of group g: toff[g] .. toff[g + 1]
  const uint32_t* tz;      // [n_terms] z mask
  const double* tcr;       // [n_terms] Re, Im of c i^#Y
  const double* tci;
};

// The sum of nblk <= kLzMaxBlocks block partials, added in index order: the block copies them into LDS (coalesced), one
// thread adds them one after the other.  The same bits in every block that asks.  stage: kLzMaxBlocks doubles of LDS.
__device__ __forceinline__ double lz_sum(const double* part, int nblk, double* stage) {
  __syncthreads();      // the readers of an earlier call are done with stage
  for (int i = threadIdx.x; i < nblk; i += kLzThreads) stage[i] = part[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int i = 0; i < nblk; ++i) acc += stage[i];
    stage[0] = acc;
  }
  __syncthreads();
  return stage[0];
}

// v = uniform draws in [-1/2, 1/2)^2 from the counter-based generator of the noise draws; block partials of |v|^2
__global__ void __launch_bounds__(kLzThreads) k_lz_start(int n, uint64_t seed, double2* v, double* pn) {
  __shared__ double red[8];
  const uint32_t dim = 1u << n;
  const uint64_t key = mix64(seed + 0x9E3779B97F4A7C15ull);
  double acc = 0.0;
  for (uint32_t base = blockIdx.x * kLzChunk; base < dim; base += gridDim.x * kLzChunk) {
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      const uint32_t p = base + threadIdx.x + (uint32_t)k * kLzThreads;
      if (p < dim) {
        const double re = (double)(mix64(key ^ ((2ull * p + 1ull) * 0x94D049BB133111EBull)) >> 11) * (1.0 / 9007199254740992.0) - 0.5;
        const double im = (double)(mix64(key ^ ((2ull * p + 2ull) * 0x94D049BB133111EBull)) >> 11) * (1.0 / 9007199254740992.0) - 0.5;
        v[p] = make_double2(re, im);
        acc += re * re + im * im;
      }
    }
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) pn[blockIdx.x] = tot;
}

// block partials of |v|^2
__global__ void __launch_bounds__(kLzThreads) k_lz_nrm2(int n, const double2* __restrict__ v, double* __restrict__ pn) {
  __shared__ double red[8];
  const uint32_t dim = 1u << n;
  double acc = 0.0;
  for (uint32_t base = blockIdx.x * kLzChunk; base < dim; base += gridDim.x * kLzChunk) {
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      const uint32_t p = base + threadIdx.x + (uint32_t)k * kLzThreads;
      if (p < dim) {
        const double2 a = v[p];
        acc += a.x * a.x + a.y * a.y;
      }
    }
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) pn[blockIdx.x] = tot;
}

// w = H v - beta_prev vprev (vprev == NULL: w = H v) and the block partials of Re <v|w>.
// (H v)[p] = sum_g d_g(p ^ x_g) v[p ^ x_g] with d_g(q) = sum_{t in g} (cr_t + i ci_t) (-1)^popc(q & z_t).
__global__ void __launch_bounds__(kLzThreads) k_lz_apply(LzHam H, int n, const double2* __restrict__ v,
                                                         const double2* __restrict__ vprev, const double* __restrict__ beta_prev,
                                                         double2* __restrict__ w, double* __restrict__ pa,
                                                         const double* __restrict__ brk) {
  __shared__ double red[8];
  if (brk[0] != 0.0) return;
  const uint32_t dim = 1u << n;
  const double bp = vprev ? *beta_prev : 0.0;
  double acc = 0.0;
  for (uint32_t base = blockIdx.x * kLzChunk; base < dim; base += gridDim.x * kLzChunk) {
    uint32_t p[kLzApt];
    bool in[kLzApt];
    double2 o[kLzApt];
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      p[k] = base + threadIdx.x + (uint32_t)k * kLzThreads;
      in[k] = p[k] < dim;
      o[k] = make_double2(0.0, 0.0);
    }
    for (int g = 0; g < H.n_groups; ++g) {
      const uint32_t x = H.gx[g];
      const int t0 = H.toff[g], t1 = H.toff[g + 1];
      uint32_t q[kLzApt];
      double2 a[kLzApt];
      double dr[kLzApt], di[kLzApt];
#pragma unroll
      for (int k = 0; k < kLzApt; ++k) {
        q[k] = p[k] ^ x;                                   // x < dim, so q < dim whenever p < dim
        a[k] = in[k] ? v[q[k]] : make_double2(0.0, 0.0);
        dr[k] = 0.0;
        di[k] = 0.0;
      }
      for (int t = t0; t < t1; ++t) {
        const uint32_t z = H.tz[t];
        const double cr = H.tcr[t], ci = H.tci[t];
#pragma unroll
        for (int k = 0; k < kLzApt; ++k) {
          const bool neg = parity32(q[k] & z);
          dr[k] += neg ? -cr : cr;
          di[k] += neg ? -ci : ci;
        }
      }
#pragma unroll
      for (int k = 0; k < kLzApt; ++k) {
        o[k].x += dr[k] * a[k].x - di[k] * a[k].y;
        o[k].y += dr[k] * a[k].y + di[k] * a[k].x;
      }
    }
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      if (in[k]) {
        const double2 own = v[p[k]];
        if (vprev) {
          const double2 b = vprev[p[k]];
          o[k].x -= bp * b.x;
          o[k].y -= bp * b.y;
        }
        w[p[k]] = o[k];
        acc += own.x * o[k].x + own.y * o[k].y;
      }
    }
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) pa[blockIdx.x] = tot;
}

// w -= alpha v, alpha the sum of the partials of k_lz_apply
__global__ void __launch_bounds__(kLzThreads) k_lz_axpy(int n, const double2* __restrict__ v, double2* __restrict__ w,
                                                        const double* __restrict__ pa, int nblk, const double* __restrict__ brk) {
  __shared__ double stage[kLzMaxBlocks];
  if (brk[0] != 0.0) return;
  const uint32_t dim = 1u << n;
  const double alpha = lz_sum(pa, nblk, stage);
  for (uint32_t base = blockIdx.x * kLzChunk; base < dim; base += gridDim.x * kLzChunk) {
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      const uint32_t p = base + threadIdx.x + (uint32_t)k * kLzThreads;
      if (p < dim) {
        const double2 a = v[p];
        double2 b = w[p];
        b.x -= alpha * a.x;
        b.y -= alpha * a.y;
        w[p] = b;
      }
    }
  }
}

// pp[k][block] = the block's part of <v_k|w>, k = 0 .. cnt-1.  The block's first chunk of w stays in registers for the
// whole loop over k; further chunks (above 20 qubits) are read again per k, from the cache.
__global__ void __launch_bounds__(kLzThreads) k_lz_proj(int n, const double2* __restrict__ V, int cnt, const double2* __restrict__ w,
                                                        double2* __restrict__ pp, const double* __restrict__ brk) {
  __shared__ double2 red[kLzProjTile][kLzThreads / 64];
  if (brk[0] != 0.0) return;
  const uint32_t dim = 1u << n;
  const uint32_t base0 = blockIdx.x * kLzChunk, step = gridDim.x * kLzChunk;
  uint32_t p[kLzApt];
  bool in[kLzApt];
  double2 w0[kLzApt];
#pragma unroll
  for (int k = 0; k < kLzApt; ++k) {
    p[k] = base0 + threadIdx.x + (uint32_t)k * kLzThreads;
    in[k] = p[k] < dim;
    w0[k] = in[k] ? w[p[k]] : make_double2(0.0, 0.0);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k0 = 0; k0 < cnt; k0 += kLzProjTile) {
    const int kt = min(kLzProjTile, cnt - k0);
    for (int kk = 0; kk < kt; ++kk) {
      const double2* vk = V + ((size_t)(k0 + kk) << n);
      double ar = 0.0, ai = 0.0;
#pragma unroll
      for (int k = 0; k < kLzApt; ++k) {
        const double2 c = in[k] ? vk[p[k]] : make_double2(0.0, 0.0);
        ar += c.x * w0[k].x + c.y * w0[k].y;       // conj(c) * w
        ai += c.x * w0[k].y - c.y * w0[k].x;
      }
      for (uint32_t base = base0 + step; base < dim; base += step) {      // dim is a multiple of the chunk here
#pragma unroll
        for (int k = 0; k < kLzApt; ++k) {
          const uint32_t q = base + threadIdx.x + (uint32_t)k * kLzThreads;
          const double2 c = vk[q], b = w[q];
          ar += c.x * b.x + c.y * b.y;
          ai += c.x * b.y - c.y * b.x;
        }
      }
      ar = wave_sum(ar);
      ai = wave_sum(ai);
      if (lane == 0) red[kk][wave] = make_double2(ar, ai);
    }
    __syncthreads();
    if ((int)threadIdx.x < kt) {
      const double2 a = red[threadIdx.x][0], b = red[threadIdx.x][1], c = red[threadIdx.x][2], d = red[threadIdx.x][3];
      pp[(size_t)(k0 + threadIdx.x) * gridDim.x + blockIdx.x] = make_double2((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y));
    }
    __syncthreads();
  }
}

// coef[k] = sum over the blocks of pp[k][.], in index order as lz_sum adds; one block per k
__global__ void __launch_bounds__(kLzThreads) k_lz_coef(const double2* __restrict__ pp, int nblk, double2* __restrict__ coef,
                                                        const double* __restrict__ brk) {
  __shared__ double2 stage[kLzMaxBlocks];
  if (brk[0] != 0.0) return;
  const double2* row = pp + (size_t)blockIdx.x * nblk;
  for (int i = threadIdx.x; i < nblk; i += kLzThreads) stage[i] = row[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double ar = 0.0, ai = 0.0;
    for (int i = 0; i < nblk; ++i) {
      ar += stage[i].x;
      ai += stage[i].y;
    }
    coef[blockIdx.x] = make_double2(ar, ai);
  }
}

// w -= sum_k coef[k] v_k and the block partials of |w|^2
__global__ void __launch_bounds__(kLzThreads) k_lz_sub(int n, const double2* __restrict__ V, int cnt, const double2* __restrict__ coef,
                                                       double2* __restrict__ w, double* __restrict__ pn, const double* __restrict__ brk) {
  __shared__ double red[8];
  if (brk[0] != 0.0) return;
  const uint32_t dim = 1u << n;
  double acc = 0.0;
  for (uint32_t base = blockIdx.x * kLzChunk; base < dim; base += gridDim.x * kLzChunk) {
    uint32_t p[kLzApt];
    bool in[kLzApt];
    double2 o[kLzApt];
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      p[k] = base + threadIdx.x + (uint32_t)k * kLzThreads;
      in[k] = p[k] < dim;
      o[k] = in[k] ? w[p[k]] : make_double2(0.0, 0.0);
    }
    for (int j = 0; j < cnt; ++j) {
      const double2 c = coef[j];
      const double2* vj = V + ((size_t)j << n);
#pragma unroll
      for (int k = 0; k < kLzApt; ++k) {
        const double2 a = in[k] ? vj[p[k]] : make_double2(0.0, 0.0);
        o[k].x -= c.x * a.x - c.y * a.y;
        o[k].y -= c.x * a.y + c.y * a.x;
      }
    }
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      if (in[k]) {
        w[p[k]] = o[k];
        acc += o[k].x * o[k].x + o[k].y * o[k].y;
      }
    }
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) pn[blockIdx.x] = tot;
}

// beta = |w| from the partials pn.  step >= 0 (a Lanczos step): alpha[step] (the sum of pa) and beta[step] are stored; a
// beta <= thresh is a breakdown: nothing is divided, brk = {1, step}.  step < 0 (a start or Ritz vector): only a zero
// vector stops, brk = {1, -1}.  Otherwise dst = w / beta (dst == NULL: the basis is full, nothing to store; dst may be w).
__global__ void __launch_bounds__(kLzThreads) k_lz_norm(int n, const double2* w, double2* dst, const double* __restrict__ pn,
                                                        const double* __restrict__ pa, int nblk, double* alpha, double* beta,
                                                        double* brk, int step, double thresh) {
  __shared__ double stage[kLzMaxBlocks];
  if (brk[0] != 0.0) return;
  const uint32_t dim = 1u << n;
  const double b = sqrt(lz_sum(pn, nblk, stage));
  if (step >= 0 && blockIdx.x == 0) {
    const double a = lz_sum(pa, nblk, stage);
    if (threadIdx.x == 0) {
      alpha[step] = a;
      beta[step] = b;
    }
  }
  const bool dead = step >= 0 ? !(b > thresh) : !(b > 0.0);
  if (dead) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      brk[1] = (double)step;
      brk[0] = 1.0;
    }
    return;
  }
  if (!dst) return;
  for (uint32_t base = blockIdx.x * kLzChunk; base < dim; base += gridDim.x * kLzChunk) {
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      const uint32_t p = base + threadIdx.x + (uint32_t)k * kLzThreads;
      if (p < dim) {
        const double2 a = w[p];
        dst[p] = make_double2(a.x / b, a.y / b);
      }
    }
  }
}

// y = sum_k s[k] v_k and the block partials of |y|^2
__global__ void __launch_bounds__(kLzThreads) k_lz_ritz(int n, const double2* __restrict__ V, int cnt, const double* __restrict__ s,
                                                        double2* __restrict__ y, double* __restrict__ pn) {
  __shared__ double red[8];
  const uint32_t dim = 1u << n;
  double acc = 0.0;
  for (uint32_t base = blockIdx.x * kLzChunk; base < dim; base += gridDim.x * kLzChunk) {
    uint32_t p[kLzApt];
    bool in[kLzApt];
    double2 o[kLzApt];
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      p[k] = base + threadIdx.x + (uint32_t)k * kLzThreads;
      in[k] = p[k] < dim;
      o[k] = make_double2(0.0, 0.0);
    }
    for (int j = 0; j < cnt; ++j) {
      const double c = s[j];
      const double2* vj = V + ((size_t)j << n);
#pragma unroll
      for (int k = 0; k < kLzApt; ++k) {
        const double2 a = in[k] ? vj[p[k]] : make_double2(0.0, 0.0);
        o[k].x += c * a.x;
        o[k].y += c * a.y;
      }
    }
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      if (in[k]) {
        y[p[k]] = o[k];
        acc += o[k].x * o[k].x + o[k].y * o[k].y;
      }
    }
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) pn[blockIdx.x] = tot;
}

// block partials of |hy - theta y|^2, theta = <y|H|y> the sum of the partials of k_lz_apply
__global__ void __launch_bounds__(kLzThreads) k_lz_resid(int n, const double2* __restrict__ y, const double2* __restrict__ hy,
                                                         const double* __restrict__ pa, int nblk, double* __restrict__ pn) {
  __shared__ double red[8];
  __shared__ double stage[kLzMaxBlocks];
  const uint32_t dim = 1u << n;
  const double theta = lz_sum(pa, nblk, stage);
  double acc = 0.0;
  for (uint32_t base = blockIdx.x * kLzChunk; base < dim; base += gridDim.x * kLzChunk) {
#pragma unroll
    for (int k = 0; k < kLzApt; ++k) {
      const uint32_t p = base + threadIdx.x + (uint32_t)k * kLzThreads;
      if (p < dim) {
        const double2 a = y[p], b = hy[p];
        const double rx = b.x - theta * a.x, ry = b.y - theta * a.y;
        acc += rx * rx + ry * ry;
      }
    }
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) pn[blockIdx.x] = tot;
}

// out = {theta, |H y - theta y|}
__global__ void __launch_bounds__(kLzThreads) k_lz_final(const double* __restrict__ pa, const double* __restrict__ pn, int nblk,
                                                         double* __restrict__ out) {
  __shared__ double stage[kLzMaxBlocks];
  const double theta = lz_sum(pa, nblk, stage);
  const double r2 = lz_sum(pn, nblk, stage);
  if (threadIdx.x == 0) {
    out[0] = theta;
    out[1] = sqrt(r2);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------

struct LzOptions {      // vqe_lanczos_opts_t, checked
  int which, max_basis, max_matvec, check_every, start_from_init;
  double tol;
  uint64_t seed;
};

// Buffers of the solver's own; the operator is uploaded for Hamiltonian version ham_ver.
struct LzWork {
  uint64_t ham_ver = ~0ull;
  DevBuf<uint32_t> gx, tz;
  DevBuf<int32_t> toff;
  DevBuf<double> tcr, tci;
  LzHam ham{};
  double hnorm = 0.0;                   // sum of |c_t|: an upper bound of |H|
  DevBufExact<double2> basis, work;     // the stored vectors; w, y, H y
  DevBuf<double> ab, pa, pn, s, out;    // alpha[m] beta[m] brk[2]; partials; Ritz coefficients; {theta, r}
  DevBuf<double2> pp, coef;
  DevBuf<double> rot;                   // vqe_lanczos_multi: the rotation S of a thick restart
  size_t vector_bytes() const { return (basis.cap + work.cap) * sizeof(double2); }
};

inline int lz_upload_ham(LzWork& W, const HamHost& H, uint64_t ham_ver, hipStream_t st, std::string& err) {
  if (W.ham_ver == ham_ver) return VQE_OK;
  std::vector<uint32_t> gx, tz;
  std::vector<int32_t> toff{0};
  std::vector<double> cr, ci;
  double hnorm = 0.0;
  for (size_t g = 0; g < H.gx_all.size(); ++g) {
    gx.push_back(H.gx_all[g]);
    for (int k : H.group_terms[g]) {
      tz.push_back((uint32_t)H.hz[k]);
      cr.push_back(H.hcr[k]);
      ci.push_back(H.hci[k]);
      hnorm += std::hypot(H.hcr[k], H.hci[k]);
    }
    toff.push_back((int32_t)tz.size());
  }
  W.ham_ver = ~0ull;
  HIP_TRY(err, W.gx.reserve(gx.size() + 1));
  HIP_TRY(err, W.toff.reserve(toff.size()));
  HIP_TRY(err, W.tz.reserve(tz.size() + 1));
  HIP_TRY(err, W.tcr.reserve(cr.size() + 1));
  HIP_TRY(err, W.tci.reserve(ci.size() + 1));
  if (!gx.empty()) HIP_TRY(err, hipMemcpyAsync(W.gx.p, gx.data(), gx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(err, hipMemcpyAsync(W.toff.p, toff.data(), toff.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (!tz.empty()) {
    HIP_TRY(err, hipMemcpyAsync(W.tz.p, tz.data(), tz.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(err, hipMemcpyAsync(W.tcr.p, cr.data(), cr.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(err, hipMemcpyAsync(W.tci.p, ci.data(), ci.size() * sizeof(double), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(err, hipStreamSynchronize(st));      // the host vectors go out of scope
  W.ham = LzHam{(int)gx.size(), W.gx.p, W.toff.p, W.tz.p, W.tcr.p, W.tci.p};
  W.hnorm = hnorm;
  W.ham_ver = ham_ver;
  return VQE_OK;
}

// The whole run on stream st, after lz_upload_ham.  free_bytes: free device memory now (the solver's own vectors are
// counted back in, so a second call has the budget of the first).  The normalised Ritz vector is left in lz_vector(W);
// *eigenvalue is its Rayleigh quotient, info = {true residual, H applications of the recurrence, restarts, status}.
inline const double2* lz_vector(const LzWork& W, int n) { return W.work.p + ((size_t)1 << n); }

inline int lz_run(LzWork& W, int n, hipStream_t st, const double2* init, const LzOptions& o, size_t free_bytes,
                  double* eigenvalue, double info[4], std::string& err) {
  const size_t dim = (size_t)1 << n;
  const int m = lz_basis_capacity(((uint64_t)free_bytes + W.vector_bytes()) / 4, n, o.max_basis);
  if (m < 2)
    return fail(err, VQE_ENOMEM, "vqe_lanczos keeps at least 2 basis vectors beside 3 work vectors of 2^n complex128: a quarter of "
                                 "the free device memory does not hold them");
  const int nblk = (int)std::min<size_t>((dim + kLzChunk - 1) / kLzChunk, (size_t)kLzMaxBlocks);
  HIP_TRY(err, W.basis.reserve((size_t)m * dim));
  HIP_TRY(err, W.work.reserve((size_t)kLzWorkVectors * dim));
  HIP_TRY(err, W.ab.reserve((size_t)2 * m + 2));
  HIP_TRY(err, W.pa.reserve(nblk));
  HIP_TRY(err, W.pn.reserve(nblk));
  HIP_TRY(err, W.s.reserve(m));
  HIP_TRY(err, W.out.reserve(2));
  HIP_TRY(err, W.pp.reserve((size_t)m * nblk));
  HIP_TRY(err, W.coef.reserve(m));
  double2* const V = W.basis.p;
  double2* const w = W.work.p;
  double2* const y = W.work.p + dim;
  double2* const hy = W.work.p + 2 * dim;
  double* const alpha = W.ab.p;
  double* const beta = W.ab.p + m;
  double* const brk = W.ab.p + 2 * m;
  const double thresh = 1e-13 * W.hnorm;      // a beta below this is rounding of an exactly invariant subspace
  const dim3 grid((unsigned)nblk), block(kLzThreads);
  const auto vec = [&](int k) { return V + (size_t)k * dim; };

  HIP_TRY(err, hipMemsetAsync(W.ab.p, 0, ((size_t)2 * m + 2) * sizeof(double), st));
  if (o.start_from_init) hipLaunchKernelGGL(k_lz_nrm2, grid, block, 0, st, n, init, W.pn.p);
  else hipLaunchKernelGGL(k_lz_start, grid, block, 0, st, n, o.seed, vec(0), W.pn.p);
  hipLaunchKernelGGL(k_lz_norm, grid, block, 0, st, n, o.start_from_init ? init : (const double2*)vec(0), vec(0),
                     (const double*)W.pn.p, (const double*)W.pa.p, nblk, alpha, beta, brk, -1, 0.0);

  const LzRule rule{o.which, m, o.max_matvec, o.tol};
  std::vector<double> ab((size_t)2 * m + 2), s((size_t)m);
  LzCounters c{0, 0, -1};
  int restarts = 0, decision = LZ_CONTINUE, ritz_dim = 0;
  double theta = 0.0;
  for (;;) {
    const int target = std::min(std::min(c.steps + o.check_every, m), c.steps + (o.max_matvec - c.matvecs));
    for (int j = c.steps; j < target; ++j) {
      hipLaunchKernelGGL(k_lz_apply, grid, block, 0, st, W.ham, n, (const double2*)vec(j), j ? (const double2*)vec(j - 1) : nullptr,
                         (const double*)(j ? beta + j - 1 : nullptr), w, W.pa.p, (const double*)brk);
      hipLaunchKernelGGL(k_lz_axpy, grid, block, 0, st, n, (const double2*)vec(j), w, (const double*)W.pa.p, nblk, (const double*)brk);
      for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(k_lz_proj, grid, block, 0, st, n, (const double2*)V, j + 1, (const double2*)w, W.pp.p, (const double*)brk);
        hipLaunchKernelGGL(k_lz_coef, dim3((unsigned)(j + 1)), block, 0, st, (const double2*)W.pp.p, nblk, W.coef.p, (const double*)brk);
        hipLaunchKernelGGL(k_lz_sub, grid, block, 0, st, n, (const double2*)V, j + 1, (const double2*)W.coef.p, w, W.pn.p,
                           (const double*)brk);
      }
      hipLaunchKernelGGL(k_lz_norm, grid, block, 0, st, n, (const double2*)w, j + 1 < m ? vec(j + 1) : nullptr, (const double*)W.pn.p,
                         (const double*)W.pa.p, nblk, alpha, beta, brk, j, thresh);
    }
    c.matvecs += target - c.steps;
    c.steps = target;
    HIP_TRY(err, hipGetLastError());
    HIP_TRY(err, hipMemcpyAsync(ab.data(), W.ab.p, ab.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(err, hipStreamSynchronize(st));
    if (ab[(size_t)2 * m] != 0.0) {
      c.broke = (int)ab[(size_t)2 * m + 1];
      if (c.broke < 0) return fail(err, VQE_EINVAL, "vqe_lanczos: the start vector is zero");
      c.matvecs -= c.steps - (c.broke + 1);      // the steps queued behind the breakdown did not run
      c.steps = c.broke + 1;
    }
    decision = lz_decide(ab.data(), ab.data() + m, rule, c, &theta, s.data(), &ritz_dim);
    if (decision == LZ_CONTINUE) continue;
    if (decision != LZ_RESTART) break;
    // explicit restart: the normalised Ritz vector becomes v_0 of the next cycle
    HIP_TRY(err, hipMemcpyAsync(W.s.p, s.data(), (size_t)ritz_dim * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lz_ritz, grid, block, 0, st, n, (const double2*)V, ritz_dim, (const double*)W.s.p, y, W.pn.p);
    hipLaunchKernelGGL(k_lz_norm, grid, block, 0, st, n, (const double2*)y, vec(0), (const double*)W.pn.p, (const double*)W.pa.p, nblk,
                       alpha, beta, brk, -1, 0.0);
    HIP_TRY(err, hipStreamSynchronize(st));      // s is rewritten at the next look
    ++restarts;
    c.steps = 0;
  }
  // the Ritz vector, its Rayleigh quotient and its true residual by one more application of H
  HIP_TRY(err, hipMemsetAsync(brk, 0, 2 * sizeof(double), st));
  HIP_TRY(err, hipMemcpyAsync(W.s.p, s.data(), (size_t)ritz_dim * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_lz_ritz, grid, block, 0, st, n, (const double2*)V, ritz_dim, (const double*)W.s.p, y, W.pn.p);
  hipLaunchKernelGGL(k_lz_norm, grid, block, 0, st, n, (const double2*)y, y, (const double*)W.pn.p, (const double*)W.pa.p, nblk, alpha,
                     beta, brk, -1, 0.0);
  hipLaunchKernelGGL(k_lz_apply, grid, block, 0, st, W.ham, n, (const double2*)y, (const double2*)nullptr, (const double*)nullptr, hy,
                     W.pa.p, (const double*)brk);
  hipLaunchKernelGGL(k_lz_resid, grid, block, 0, st, n, (const double2*)y, (const double2*)hy, (const double*)W.pa.p, nblk, W.pn.p);
  hipLaunchKernelGGL(k_lz_final, dim3(1), block, 0, st, (const double*)W.pa.p, (const double*)W.pn.p, nblk, W.out.p);
  HIP_TRY(err, hipGetLastError());
  double out[2] = {0.0, 0.0};
  HIP_TRY(err, hipMemcpyAsync(out, W.out.p, sizeof(out), hipMemcpyDeviceToHost, st));
  HIP_TRY(err, hipStreamSynchronize(st));
  *eigenvalue = out[0];
  info[0] = out[1];
  info[1] = (double)c.matvecs;
  info[2] = (double)restarts;
  info[3] = decision == LZ_CONVERGED ? 0.0 : (decision == LZ_BREAKDOWN ? 1.0 : 2.0);
  return VQE_OK;
}

// ---- several eigenpairs: thick restart, locking by deflation (vqe_lanczos_multi) -------------------------------
// Locked eigenvectors sit in basis slots 0 .. e-1, the active basis of stage e behind them; k_lz_proj / k_lz_coef /
// k_lz_sub run over (V, e + j + 1), so the full reorthogonalisation deflates the locked vectors as it goes.  The stage /
// look / restart / lock logic is LzMulti (lanczos_host.h); lz_run_multi executes its commands with the kernels above and
// the one below.

constexpr size_t kLzRotLds = 32768;        // bytes of LDS a block of k_lz_rotate stages: 4 blocks on a CU's 160 KiB
constexpr int kLzRotQ = 4;                 // outputs a thread accumulates from one LDS read
constexpr int kLzRotMaxBlocks = 4096;
static_assert((size_t)kLzMaxActive * sizeof(double2) <= kLzRotLds, "a block of k_lz_rotate stages at least one amplitude of every vector");

// The thick restart, in place over the m active vectors A[i] = A + i 2^n:  A[q] <- sum_i S[i][q] A[i] for q < r (S real,
// S[i][q] = S[i * ld + q], rows padded with zeros to ld = a multiple of kLzRotQ), and A[r] <- resid where resid != NULL.
// A block stages a chunk of C = 2^lc amplitudes of all m vectors in LDS (m C 16 bytes <= kLzRotLds; [i][c], so a wave
// reads consecutive 16-byte words), then writes the r outputs of that chunk: every input of an amplitude is read before
// any of its outputs is written, and no other block touches the chunk.  Thread t owns amplitude t mod C and the output
// groups q0 = kLzRotQ (t / C), + kLzRotQ 256 / C, ..; sums over i ascending, no atomics.
__global__ void __launch_bounds__(kLzThreads) k_lz_rotate(int n, double2* A, int m, int r, int ld, const double* __restrict__ S,
                                                          const double2* __restrict__ resid, int lc) {
  extern __shared__ double2 lz_rot[];
  const uint32_t dim = 1u << n;
  const uint32_t C = 1u << lc;
  const uint32_t c = threadIdx.x & (C - 1u);
  const int grp = (int)(threadIdx.x >> lc), ngrp = kLzThreads >> lc;
  const int total = m << lc;
  for (uint32_t base = blockIdx.x * C; base < dim; base += gridDim.x * C) {
    __syncthreads();      // the readers of the previous chunk are done with the stage
    for (int t = threadIdx.x; t < total; t += kLzThreads) {
      const uint32_t p = base + ((uint32_t)t & (C - 1u));
      lz_rot[t] = p < dim ? A[((size_t)(t >> lc) << n) + p] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const uint32_t p = base + c;
    if (p < dim) {
      for (int q0 = grp * kLzRotQ; q0 < r; q0 += ngrp * kLzRotQ) {
        double2 acc[kLzRotQ];
#pragma unroll
        for (int k = 0; k < kLzRotQ; ++k) acc[k] = make_double2(0.0, 0.0);
        const double* row = S + q0;
        for (int i = 0; i < m; ++i, row += ld) {
          const double2 a = lz_rot[((uint32_t)i << lc) + c];
#pragma unroll
          for (int k = 0; k < kLzRotQ; ++k) {
            acc[k].x += row[k] * a.x;
            acc[k].y += row[k] * a.y;
          }
        }
#pragma unroll
        for (int k = 0; k < kLzRotQ; ++k)
          if (q0 + k < r) A[((size_t)(q0 + k) << n) + p] = acc[k];
      }
      if (resid && grp == 0) A[((size_t)r << n) + p] = resid[p];
    }
  }
}

// log2 of the chunk of k_lz_rotate for m active vectors: the largest power of two with m C 16 <= kLzRotLds, C <= 256
inline int lz_rotate_chunk_log2(int m) {
  int lc = 0;
  while (lc < 8 && ((size_t)m << (lc + 1)) * sizeof(double2) <= kLzRotLds) ++lc;
  return lc;
}

// The whole run on stream st, after lz_upload_ham.  The eigenvectors are left in the basis slots; pair i of the answer
// (eigenvalues ascending for which = 0, descending for which = 1) is lz_multi_vector(W, n, order[i]).
// info = {largest true residual, H applications of the recurrences, restarts, status, pairs returned}.
inline const double2* lz_multi_vector(const LzWork& W, int n, int slot) { return W.basis.p + ((size_t)slot << n); }

inline int lz_run_multi(LzWork& W, int n, hipStream_t st, const LzMultiOptions& o, size_t free_bytes, double* eigenvalues,
                        double* residuals, int* order, double info[5], std::string& err) {
  const size_t dim = (size_t)1 << n;
  const int M = lz_multi_slots(((uint64_t)free_bytes + W.vector_bytes()) / 4, n, o.max_basis, o.n_eig);
  if (!lz_multi_fits(M, n, o.max_basis, o.n_eig))
    return fail(err, VQE_ENOMEM, "vqe_lanczos_multi keeps n_eig - 1 locked vectors and at least 2 active basis vectors beside 3 work "
                                 "vectors of 2^n complex128: a quarter of the free device memory does not hold them");
  const int capmax = lz_stage_capacity(M, n, o.max_basis, 0);
  const int nblk = (int)std::min<size_t>((dim + kLzChunk - 1) / kLzChunk, (size_t)kLzMaxBlocks);
  HIP_TRY(err, W.basis.reserve((size_t)M * dim));
  HIP_TRY(err, W.work.reserve((size_t)kLzWorkVectors * dim));
  HIP_TRY(err, W.ab.reserve((size_t)2 * capmax + 2));
  HIP_TRY(err, W.pa.reserve(nblk));
  HIP_TRY(err, W.pn.reserve(nblk));
  HIP_TRY(err, W.s.reserve(capmax));
  HIP_TRY(err, W.rot.reserve((size_t)capmax * (capmax + kLzRotQ)));
  HIP_TRY(err, W.out.reserve(2));
  HIP_TRY(err, W.pp.reserve((size_t)M * nblk));
  HIP_TRY(err, W.coef.reserve(M));
  double2* const V = W.basis.p;
  double2* const w = W.work.p;
  double2* const y = W.work.p + dim;
  double2* const hy = W.work.p + 2 * dim;
  double* const alpha = W.ab.p;
  double* const beta = W.ab.p + capmax;
  double* const brk = W.ab.p + 2 * capmax;
  const double thresh = 1e-13 * W.hnorm;
  const dim3 grid((unsigned)nblk), block(kLzThreads);
  const auto vec = [&](int k) { return V + (size_t)k * dim; };
  const auto orthogonalise = [&](int cnt) {      // two passes of classical Gram-Schmidt of w against slots 0 .. cnt-1
    for (int pass = 0; pass < 2; ++pass) {
      hipLaunchKernelGGL(k_lz_proj, grid, block, 0, st, n, (const double2*)V, cnt, (const double2*)w, W.pp.p, (const double*)brk);
      hipLaunchKernelGGL(k_lz_coef, dim3((unsigned)cnt), block, 0, st, (const double2*)W.pp.p, nblk, W.coef.p, (const double*)brk);
      hipLaunchKernelGGL(k_lz_sub, grid, block, 0, st, n, (const double2*)V, cnt, (const double2*)W.coef.p, w, W.pn.p, (const double*)brk);
    }
  };

  std::vector<double> ab((size_t)2 * capmax + 2);
  LzMulti mach(o, n, M);
  for (;;) {
    const LzMultiCmd c = mach.cmd();
    if (c.op == LZM_DONE) break;
    const int e = c.stage;
    if (c.op == LZM_START) {
      HIP_TRY(err, hipMemsetAsync(W.ab.p, 0, ((size_t)2 * capmax + 2) * sizeof(double), st));
      hipLaunchKernelGGL(k_lz_start, grid, block, 0, st, n, c.seed, w, W.pn.p);
      if (e > 0) orthogonalise(e);
      hipLaunchKernelGGL(k_lz_norm, grid, block, 0, st, n, (const double2*)w, vec(e), (const double*)W.pn.p, (const double*)W.pa.p, nblk,
                         alpha, beta, brk, -1, 0.0);
      mach.started();
    } else if (c.op == LZM_STEPS) {
      for (int j = c.j0; j < c.j1; ++j) {
        const bool prev = !(j == c.j0 && c.no_prev);
        hipLaunchKernelGGL(k_lz_apply, grid, block, 0, st, W.ham, n, (const double2*)vec(e + j),
                           prev ? (const double2*)vec(e + j - 1) : nullptr, (const double*)(prev ? beta + j - 1 : nullptr), w, W.pa.p,
                           (const double*)brk);
        hipLaunchKernelGGL(k_lz_axpy, grid, block, 0, st, n, (const double2*)vec(e + j), w, (const double*)W.pa.p, nblk, (const double*)brk);
        orthogonalise(e + j + 1);
        hipLaunchKernelGGL(k_lz_norm, grid, block, 0, st, n, (const double2*)w, j + 1 < c.capacity ? vec(e + j + 1) : w,
                           (const double*)W.pn.p, (const double*)W.pa.p, nblk, alpha, beta, brk, j, thresh);
      }
      HIP_TRY(err, hipGetLastError());
      HIP_TRY(err, hipMemcpyAsync(ab.data(), W.ab.p, ab.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(err, hipStreamSynchronize(st));
      int broke = -1;
      if (ab[(size_t)2 * capmax] != 0.0) {
        broke = (int)ab[(size_t)2 * capmax + 1];
        if (broke < 0) return fail(err, VQE_EINVAL, "vqe_lanczos_multi: the start vector of a stage is zero");
      }
      mach.steps_done(ab.data(), ab.data() + capmax, broke);
    } else if (c.op == LZM_RESTART) {
      const int lc = lz_rotate_chunk_log2(c.m);
      const size_t chunks = (dim + ((size_t)1 << lc) - 1) >> lc;
      HIP_TRY(err, hipMemcpyAsync(W.rot.p, c.s, (size_t)c.m * c.ld * sizeof(double), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_lz_rotate, dim3((unsigned)std::min<size_t>(chunks, (size_t)kLzRotMaxBlocks)), block,
                         ((size_t)c.m << lc) * sizeof(double2), st, n, vec(e), c.m, c.r, c.ld, (const double*)W.rot.p,
                         c.with_resid ? (const double2*)w : nullptr, lc);
      HIP_TRY(err, hipGetLastError());
      HIP_TRY(err, hipStreamSynchronize(st));      // S is rebuilt at the next restart
      mach.restarted();
    } else {      // LZM_LOCK: the Ritz vector into slot e, its Rayleigh quotient and true residual by one more application
      HIP_TRY(err, hipMemsetAsync(brk, 0, 2 * sizeof(double), st));
      HIP_TRY(err, hipMemcpyAsync(W.s.p, c.s, (size_t)c.m * sizeof(double), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_lz_ritz, grid, block, 0, st, n, (const double2*)vec(e), c.m, (const double*)W.s.p, y, W.pn.p);
      hipLaunchKernelGGL(k_lz_norm, grid, block, 0, st, n, (const double2*)y, vec(e), (const double*)W.pn.p, (const double*)W.pa.p, nblk,
                         alpha, beta, brk, -1, 0.0);
      hipLaunchKernelGGL(k_lz_apply, grid, block, 0, st, W.ham, n, (const double2*)vec(e), (const double2*)nullptr, (const double*)nullptr,
                         hy, W.pa.p, (const double*)brk);
      hipLaunchKernelGGL(k_lz_resid, grid, block, 0, st, n, (const double2*)vec(e), (const double2*)hy, (const double*)W.pa.p, nblk, W.pn.p);
      hipLaunchKernelGGL(k_lz_final, dim3(1), block, 0, st, (const double*)W.pa.p, (const double*)W.pn.p, nblk, W.out.p);
      HIP_TRY(err, hipGetLastError());
      double out[2] = {0.0, 0.0};
      HIP_TRY(err, hipMemcpyAsync(out, W.out.p, sizeof(out), hipMemcpyDeviceToHost, st));
      HIP_TRY(err, hipStreamSynchronize(st));
      mach.locked(out[0], out[1]);
    }
  }
  const int pairs = mach.pairs();
  for (int i = 0; i < pairs; ++i) order[i] = i;
  std::stable_sort(order, order + pairs, [&](int a, int b) { return o.which ? mach.theta(a) > mach.theta(b) : mach.theta(a) < mach.theta(b); });
  double worst = 0.0;
  for (int i = 0; i < o.n_eig; ++i) {
    eigenvalues[i] = i < pairs ? mach.theta(order[i]) : std::numeric_limits<double>::quiet_NaN();
    residuals[i] = i < pairs ? mach.residual(order[i]) : std::numeric_limits<double>::quiet_NaN();
    if (i < pairs) worst = std::max(worst, residuals[i]);
  }
  info[0] = worst;
  info[1] = (double)mach.matvecs();
  info[2] = (double)mach.restarts();
  info[3] = (double)mach.status();
  info[4] = (double)pairs;
  return VQE_OK;
}

}  // namespace vqe
