// mps2qc_resident_kernels.h - the resident streaming fit (mps2qc_fit_brickwork_resident): the streaming fit of
// mps2qc_fit.hip with the Stiefel-Adam update and the bookkeeping of minimize() on the device.  Included by
// mps2qc_fit.hip after the host-update path, whose arithmetic helpers (cmul, block_sum_sf, ...) and host layer
// (begin_fit, upload, download, the owners) it uses; the k_sf_* kernels and SfHost are not touched.
//
// Per-fit device state: active[b], it[b], bv[b], the gates, best gates, both moments, the loss history, the
// environments and the overlap.  One step is the fixed sequence
//   zero state, G x apply, dot, copy target -> phi, G x back, reduce_all, update        (2 G + 5 launches, no copy)
// which does not depend on the step number (the update reads lr_t[it[b]] from a table), so one captured graph - a
// linear chain - serves every replay.  Every block of fit b reads active[b] first and returns when it is 0: a fit that
// has stopped costs no bandwidth and its outputs stay those of its last executed step; the update clears active[b] when
// it[b] reaches max_iter, so replays past the budget do nothing.
#pragma once
#include "mps2qc_resident.h"

namespace {

static_assert(kSfdThreads == kSfThreads, "block_sum_sf folds the four waves of a 256-thread block");

// dst[t][i] = src[t][little_endian ? bitrev_n(i) : i]: the fit's own copy of the target(s), in quimb's order
__global__ void __launch_bounds__(kSfdThreads) k_sfd_load_target(double2* dst, const double2* src, size_t dim, int n,
                                                                 int little_endian) {
  const size_t i = (size_t)blockIdx.x * kSfdThreads + threadIdx.x;
  if (i >= dim) return;
  const size_t t = (size_t)blockIdx.y * dim;
  dst[t + i] = src[t + (little_endian ? sfd_bitrev(i, n) : i)];
}

__global__ void __launch_bounds__(kSfdThreads) k_sfd_zero_state(const int* active, double2* psi, size_t dim) {
  if (!active[blockIdx.y]) return;
  const size_t i = (size_t)blockIdx.x * kSfdThreads + threadIdx.x;
  if (i < dim) psi[(size_t)blockIdx.y * dim + i] = make_double2(i == 0 ? 1.0 : 0.0, 0.0);
}

__global__ void __launch_bounds__(kSfdThreads) k_sfd_copy(const int* active, double2* dst, const double2* src, size_t dim,
                                                          int src_shared) {
  if (!active[blockIdx.y]) return;
  const size_t i = (size_t)blockIdx.x * kSfdThreads + threadIdx.x;
  if (i < dim) dst[(size_t)blockIdx.y * dim + i] = src[(src_shared ? 0 : (size_t)blockIdx.y * dim) + i];
}

// psi <- U_k psi on the qubit pair with low bit `lo` (the arithmetic of k_sf_apply)
__global__ void __launch_bounds__(kSfdThreads) k_sfd_apply(const int* active, double2* states, size_t dim, const double2* gates,
                                                           int G, int k, int lo) {
  if (!active[blockIdx.y]) return;
  const size_t r = (size_t)blockIdx.x * kSfdThreads + threadIdx.x;
  if (r >= dim / 4) return;
  double2* st = states + (size_t)blockIdx.y * dim;
  const double2* M = gates + ((size_t)blockIdx.y * G + k) * kMat;
  const size_t base = ((r >> lo) << (lo + 2)) | (r & (((size_t)1 << lo) - 1));
  double2 v[4], w[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) v[b] = st[base | ((size_t)b << lo)];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    double2 s = cmul(M[a * 4], v[0]);
#pragma unroll
    for (int b = 1; b < 4; ++b) s = cmac(s, M[a * 4 + b], v[b]);
    w[a] = s;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) st[base | ((size_t)a << lo)] = w[a];
}

// partial[b][block] = sum over the block's amplitudes of conj(t) psi
__global__ void __launch_bounds__(kSfdThreads) k_sfd_dot(const int* active, const double2* target, int target_shared,
                                                         const double2* psi, size_t dim, double2* partial) {
  __shared__ double red[4];
  if (!active[blockIdx.y]) return;
  const size_t i = (size_t)blockIdx.x * kSfdThreads + threadIdx.x;
  const double2* t = target + (target_shared ? 0 : (size_t)blockIdx.y * dim);
  const double2* p = psi + (size_t)blockIdx.y * dim;
  double2 c = make_double2(0.0, 0.0);
  if (i < dim) c = cmulc(p[i], t[i]);
  const double x = block_sum_sf(c.x, red), y = block_sum_sf(c.y, red);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = make_double2(x, y);
}

// fused backward step of gate k (the arithmetic of k_sf_back): psi <- U^H psi, E[a][b] += conj(phi[a]) psi[b],
// phi <- U^H phi; the block's 16 partials go to partial[b][k][block][16]
__global__ void __launch_bounds__(kSfdThreads) k_sfd_back(const int* active, double2* psi_all, double2* phi_all, size_t dim,
                                                          const double2* gates, int G, int k, int lo, double2* partial) {
  __shared__ double red[4];
  if (!active[blockIdx.y]) return;
  const size_t r = (size_t)blockIdx.x * kSfdThreads + threadIdx.x;
  double2* psi = psi_all + (size_t)blockIdx.y * dim;
  double2* phi = phi_all + (size_t)blockIdx.y * dim;
  const double2* M = gates + ((size_t)blockIdx.y * G + k) * kMat;
  double2 e[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) e[q] = make_double2(0.0, 0.0);
  if (r < dim / 4) {
    const size_t base = ((r >> lo) << (lo + 2)) | (r & (((size_t)1 << lo) - 1));
    double2 p[4], f[4], pw[4], fw[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) { p[b] = psi[base | ((size_t)b << lo)]; f[b] = phi[base | ((size_t)b << lo)]; }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double2 sp = make_double2(0.0, 0.0), sf = make_double2(0.0, 0.0);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        double2 m = M[b * 4 + a];
        m.y = -m.y;                                   // (U^H)[a][b] = conj(U[b][a])
        sp = b == 0 ? cmul(m, p[0]) : cmac(sp, m, p[b]);
        sf = b == 0 ? cmul(m, f[0]) : cmac(sf, m, f[b]);
      }
      pw[a] = sp; fw[a] = sf;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) e[a * 4 + b] = cmulc(pw[b], f[a]);
#pragma unroll
    for (int a = 0; a < 4; ++a) { psi[base | ((size_t)a << lo)] = pw[a]; phi[base | ((size_t)a << lo)] = fw[a]; }
  }
  double2* out = partial + ((((size_t)blockIdx.y * G + k) * gridDim.x) + blockIdx.x) * 16;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const double x = block_sum_sf(e[q].x, red), y = block_sum_sf(e[q].y, red);
    if (threadIdx.x == 0) out[q] = make_double2(x, y);
  }
}

// All second-stage reductions of a step, grid (G + 1, B): slot G the overlap, slots 0 .. G-1 the 16 environment entries
// of a gate.  Fixed order, that of k_sf_reduce: thread-strided over the blocks, then block_sum_sf.  A thread reads the
// whole 256-byte row of a block once and keeps the 16 running sums in registers.
__global__ void __launch_bounds__(kSfdThreads) k_sfd_reduce_all(const int* active, const double2* part_env, size_t nblk_vec,
                                                                const double2* part_ov, size_t nblk_amp, int G, double2* env,
                                                                double2* ov) {
  __shared__ double red[4];
  const size_t b = blockIdx.y;
  if (!active[b]) return;
  const int slot = blockIdx.x;
  if (slot == G) {
    double x = 0.0, y = 0.0;
    for (size_t i = threadIdx.x; i < nblk_amp; i += kSfdThreads) {
      const double2 v = part_ov[b * nblk_amp + i];
      x += v.x; y += v.y;
    }
    x = block_sum_sf(x, red); y = block_sum_sf(y, red);
    if (threadIdx.x == 0) ov[b] = make_double2(x, y);
    return;
  }
  const double2* rows = part_env + (b * G + slot) * nblk_vec * 16;
  double2 s[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) s[q] = make_double2(0.0, 0.0);
  for (size_t i = threadIdx.x; i < nblk_vec; i += kSfdThreads) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const double2 v = rows[i * 16 + q];
      s[q].x += v.x; s[q].y += v.y;
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const double x = block_sum_sf(s[q].x, red), y = block_sum_sf(s[q].y, red);
    if (threadIdx.x == 0) env[(b * G + slot) * kMat + q] = make_double2(x, y);
  }
}

// ---- StiefelAdam.update on 16-lane groups --------------------------------------------------------------------------
// Lane e = 4 i + j of a group holds element (i, j) of every 4x4 matrix of one gate's update; `gb` is the group's first
// lane in the wavefront.  An operand of a product comes from the lane that holds it (ds_bpermute), so no matrix is ever
// an array indexed at run time.  EVERY lane of a wavefront must execute every one of these calls: a shuffle that reads
// a lane which is not executing returns garbage.
__device__ __forceinline__ double2 sfd_lane(double2 v, int src) {
  return make_double2(__shfl(v.x, src, 64), __shfl(v.y, src, 64));
}
__device__ __forceinline__ double2 sfd_mm(double2 a, double2 b, int gb, int i, int j) {      // (A B)[i][j]
  double2 s = make_double2(0.0, 0.0);
#pragma unroll
  for (int l = 0; l < 4; ++l) s = cadd(s, cmul(sfd_lane(a, gb + i * 4 + l), sfd_lane(b, gb + l * 4 + j)));
  return s;
}
__device__ __forceinline__ double2 sfd_mmh(double2 a, double2 b, int gb, int i, int j) {     // (A B^H)[i][j]
  double2 s = make_double2(0.0, 0.0);
#pragma unroll
  for (int l = 0; l < 4; ++l) s = cadd(s, cmulc(sfd_lane(a, gb + i * 4 + l), sfd_lane(b, gb + j * 4 + l)));
  return s;
}
__device__ __forceinline__ double sfd_group_sum(double v) {      // fixed-order xor reduction over the 16 lanes
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += shfl_xor_d(v, m);
  return v;
}

struct SfdUpdateArgs {
  int G, max_iter, frozen;
  double beta1, beta2, eps, tol, param_tol;
  const double* lr_t;      // [max_iter]
  double2 *env, *ov;       // [B][G][16], [B]: written by k_sfd_reduce_all
  double2 *gates, *best, *mom, *vel;      // [B][G][16]
  double *hist, *bv;       // [B][max_iter], [B]
  int *it, *active;        // [B]
};

// grid B: SfHost::host_step of fit blockIdx.x.  Four gates per wavefront, sixteen per pass of the workgroup; the pass
// count is the same for every lane, and a lane whose gate index is >= G computes on gate 0 and masks its stores.
__global__ void __launch_bounds__(kSfdThreads) k_sfd_update(SfdUpdateArgs A) {
  extern __shared__ double dnorm[];      // [G]
  const int b = blockIdx.x;
  if (!A.active[b]) return;
  const int tid = threadIdx.x, e = tid & 15, i = e >> 2, j = e & 3, gb = tid & 48, grp = tid >> 4;
  const int G = A.G, it = A.it[b];
  const size_t gbase = (size_t)b * G * kMat;
  const double lr = A.lr_t[it];
  const double2 o = A.ov[b];
  const double ao = hypot(o.x, o.y), val = 1.0 - ao;
  const double2 ph = make_double2(o.x / ao, o.y / ao);
  const bool improved = val < A.bv[b];
  const double dg = i == j ? 1.0 : 0.0;

  for (int k0 = 0; k0 < G; k0 += kSfdThreads / 16) {
    const int k = k0 + grp;
    const bool act = k < G;
    const size_t at = gbase + (size_t)(act ? k : 0) * kMat + e;
    const double2 u = A.gates[at], E = A.env[at];
    const double2 pe = cmul(ph, make_double2(E.x, -E.y));
    const double2 g = make_double2(-pe.x, -pe.y);                       // -(o/|o|) conj(E_k)
    const double2 rg = csub(g, sfd_mm(sfd_mmh(u, g, gb, i, j), u, gb, i, j));      // g - p g^H p
    const double tr = sfd_group_sum(rg.x * rg.x + rg.y * rg.y);         // Re tr(rg^H rg)
    double2 m0 = make_double2(0.0, 0.0), v0 = make_double2(0.0, 0.0);
    if (!A.frozen) { m0 = A.mom[at]; v0 = A.vel[at]; }
    const double2 mom = make_double2(A.beta1 * m0.x + (1 - A.beta1) * rg.x, A.beta1 * m0.y + (1 - A.beta1) * rg.y);
    const double2 vel = make_double2(A.beta2 * v0.x + (1 - A.beta2) * tr, A.beta2 * v0.y);
    double2 den = csqrt_principal(vel);
    den.x += A.eps;
    const double2 dir = cscale(-lr, cmul(mom, cinv(den)));
    // Cayley retraction: a = g' p^H - p g'^H, new = (I - a/2)^-1 (I + a/2) p
    const double2 a = csub(sfd_mmh(dir, u, gb, i, j), sfd_mmh(u, dir, gb, i, j));
    double2 mm = make_double2(dg - 0.5 * a.x, -0.5 * a.y);
    double2 y = sfd_mm(make_double2(dg + 0.5 * a.x, 0.5 * a.y), u, gb, i, j);
#pragma unroll
    for (int pv = 0; pv < 4; ++pv) {      // Gauss-Jordan without pivoting: the Hermitian part of (I - a/2) is the identity
      const double2 inv = cinv(sfd_lane(mm, gb + pv * 4 + pv));
      const double2 mrow = sfd_lane(mm, gb + pv * 4 + j), yrow = sfd_lane(y, gb + pv * 4 + j);
      const double2 f = cmul(sfd_lane(mm, gb + i * 4 + pv), inv);
      if (i == pv) {
        mm = cmul(mrow, inv);
        y = cmul(yrow, inv);
      } else {
        mm = csub(mm, cmul(f, mrow));
        y = csub(y, cmul(f, yrow));
      }
    }
    const double df = sfd_group_sum((y.x - u.x) * (y.x - u.x) + (y.y - u.y) * (y.y - u.y));
    if (!A.frozen) {      // vector transport 0.5 (M - U M^H U) of both moments
      const double2 tm = sfd_mm(sfd_mmh(y, mom, gb, i, j), y, gb, i, j), tv = sfd_mm(sfd_mmh(y, vel, gb, i, j), y, gb, i, j);
      if (act) {
        A.mom[at] = make_double2(0.5 * (mom.x - tm.x), 0.5 * (mom.y - tm.y));
        A.vel[at] = make_double2(0.5 * (vel.x - tv.x), 0.5 * (vel.y - tv.y));
      }
    }
    if (act) {
      A.gates[at] = y;
      if (improved) A.best[at] = y;
      if (e == 0) dnorm[k] = sqrt(df);
    }
  }
  __syncthreads();
  if (tid == 0) {      // bookkeeping of minimize(); the norms are summed in gate order, as the host path does
    double dsum = 0.0;
    for (int k = 0; k < G; ++k) dsum += dnorm[k];
    A.hist[(size_t)b * A.max_iter + it] = val;
    A.it[b] = it + 1;
    if (improved) A.bv[b] = val;
    if (val < A.tol || dsum / G < A.param_tol || it + 1 >= A.max_iter) A.active[b] = 0;
  }
}

// One step on the stream, and its graph
struct SfdStep {
  int B, G, target_shared;
  size_t dim, nblk_amp, nblk_vec;
  const int* lo;                                   // [G], host
  int* active;                                     // device
  double2 *psi, *phi, *tgt, *part_env, *part_ov;   // device
  SfdUpdateArgs U;
  Graph graph;
  GraphExec exec;

  hipError_t enqueue(hipStream_t st) const {
    const dim3 amp((unsigned)nblk_amp, B), vec((unsigned)nblk_vec, B), nt(kSfdThreads);
    hipLaunchKernelGGL(k_sfd_zero_state, amp, nt, 0, st, active, psi, dim);
    for (int k = 0; k < G; ++k) hipLaunchKernelGGL(k_sfd_apply, vec, nt, 0, st, active, psi, dim, U.gates, G, k, lo[k]);
    hipLaunchKernelGGL(k_sfd_dot, amp, nt, 0, st, active, tgt, target_shared, psi, dim, part_ov);
    hipLaunchKernelGGL(k_sfd_copy, amp, nt, 0, st, active, phi, tgt, dim, target_shared);
    for (int k = G - 1; k >= 0; --k)
      hipLaunchKernelGGL(k_sfd_back, vec, nt, 0, st, active, psi, phi, dim, U.gates, G, k, lo[k], part_env);
    hipLaunchKernelGGL(k_sfd_reduce_all, dim3(G + 1, B), nt, 0, st, active, part_env, nblk_vec, part_ov, nblk_amp, G,
                       U.env, U.ov);
    hipLaunchKernelGGL(k_sfd_update, dim3(B), nt, (size_t)G * sizeof(double), st, U);
    return hipGetLastError();
  }
  // st must be idle.  A capture that fails is dropped without a word: run() then enqueues plain launches.
  void capture(hipStream_t st) {
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
      const hipError_t e = enqueue(st), e2 = hipStreamEndCapture(st, &graph.h);
      if (e == hipSuccess && e2 == hipSuccess && graph.h && hipGraphInstantiate(&exec.h, graph.h, nullptr, nullptr, 0) == hipSuccess) return;
      exec.h = nullptr;
    }
    (void)hipGetLastError();
  }
  hipError_t run(hipStream_t st) const { return exec.h ? hipGraphLaunch(exec.h, st) : enqueue(st); }
};

// target_on_device = 1: the pointer must be device memory of device_id
bool sfd_is_device_memory(const void* p, int device_id) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeDevice && at.device == device_id;
}

}  // namespace

extern "C" int mps2qc_resident_default_opts(mps2qc_resident_opts_t* o) {
  if (!o) return fail(ErrOut{}, VQE_EINVAL, "mps2qc_resident_default_opts: null argument");
  *o = sfd_default_opts();
  return 0;
}

extern "C" int mps2qc_fit_brickwork_resident(int device_id, int n, int G, const int32_t* sites, int batch, const void* target,
                                             int target_shared, const double* init_gates, double lr, double beta1,
                                             double beta2, double eps, int jit_frozen, int max_iter, double tol,
                                             double param_tol, const mps2qc_resident_opts_t* opts, double* opt_gates,
                                             double* final_gates, double* loss_history, double* best_val, int32_t* n_iter,
                                             double* last_envs, double* last_overlap, float* total_ms,
                                             int32_t* steps_enqueued) {
  ErrOut err;
  std::vector<int> lo;
  VQE_TRY(begin_fit("mps2qc_fit_brickwork_resident", MPS2QC_STREAM_MAX_QUBITS, device_id, n, G, batch, max_iter, sites, target,
                    init_gates, lo));
  const mps2qc_resident_opts_t O = opts ? *opts : sfd_default_opts();
  std::string msg;
  if (!sfd_check_opts(O, msg)) return fail(err, VQE_EINVAL, msg);
  HIP_TRY(err, hipSetDevice(device_id));
  if (O.target_on_device && !sfd_is_device_memory(target, device_id))
    return fail(err, VQE_EINVAL, "mps2qc_fit_brickwork_resident: target_on_device = 1, but target is not device memory of device " +
                                     std::to_string(device_id));
  const bool use_graph = O.use_graph < 0 ? read_knobs(true).stream_graph : O.use_graph != 0;
  const size_t dim = (size_t)1 << n, gcount = (size_t)batch * G * kMat, hcount = (size_t)batch * max_iter;
  const int n_targets = target_shared ? 1 : batch;
  const size_t tcount = (size_t)n_targets * dim;
  std::vector<double> lr_t(max_iter);
  for (int it = 0; it < max_iter; ++it) lr_t[it] = lr_schedule(lr, beta1, beta2, jit_frozen != 0, it);
  const std::vector<int> ones(batch, 1);
  const std::vector<double> bv0(batch, 10000.0);      // stiefel_opt.py:122

  // allocate and upload
  Stream st;
  Event e0, e1;
  Pinned pin;
  SfdStep S;
  DevBufExact<int> d_act, d_it;
  DevBufExact<double> d_lr, d_hist, d_bv;
  DevBufExact<double2> d_psi, d_phi, d_t, d_raw, d_g, d_best, d_m, d_v, d_env, d_ov, d_penv, d_pov;
  HIP_TRY(err, hipStreamCreate(&st.h));
  HIP_TRY(err, hipEventCreate(&e0.h));
  HIP_TRY(err, hipEventCreate(&e1.h));
  HIP_TRY(err, hipHostMalloc(&pin.h, (size_t)batch * sizeof(int), hipHostMallocDefault));
  HIP_TRY(err, d_psi.reserve(sfd_state_count(n, batch)));
  HIP_TRY(err, d_phi.reserve(sfd_state_count(n, batch)));
  HIP_TRY(err, d_penv.reserve(sfd_env_partial_count(n, G, batch)));
  HIP_TRY(err, d_pov.reserve(sfd_ov_partial_count(n, batch)));
  HIP_TRY(err, d_env.reserve(gcount));
  HIP_TRY(err, d_ov.reserve(batch));
  HIP_TRY(err, d_it.reserve(batch));
  HIP_TRY(err, d_hist.reserve(hcount));
  for (DevBufExact<double2>* b : {&d_m, &d_v}) {
    HIP_TRY(err, b->reserve(gcount));
    HIP_TRY(err, hipMemsetAsync(b->p, 0, gcount * sizeof(double2), st.h));
  }
  HIP_TRY(err, hipMemsetAsync(d_env.p, 0, gcount * sizeof(double2), st.h));
  HIP_TRY(err, hipMemsetAsync(d_ov.p, 0, (size_t)batch * sizeof(double2), st.h));
  HIP_TRY(err, hipMemsetAsync(d_it.p, 0, (size_t)batch * sizeof(int), st.h));
  HIP_TRY(err, hipMemsetAsync(d_hist.p, 0, hcount * sizeof(double), st.h));
  VQE_TRY(upload(d_act, ones.data(), batch, st.h));
  VQE_TRY(upload(d_bv, bv0.data(), batch, st.h));
  VQE_TRY(upload(d_lr, lr_t.data(), max_iter, st.h));
  VQE_TRY(upload(d_g, init_gates, gcount, st.h));
  VQE_TRY(upload(d_best, init_gates, gcount, st.h));
  // the target: a host target in quimb's order goes straight into the fit's buffer, every other one through k_sfd_load_target
  if (!O.target_on_device && !O.target_little_endian) {
    VQE_TRY(upload(d_t, target, tcount, st.h));
  } else {
    const double2* src = static_cast<const double2*>(target);
    if (!O.target_on_device) {
      VQE_TRY(upload(d_raw, target, tcount, st.h));
      src = d_raw.p;
    }
    HIP_TRY(err, d_t.reserve(tcount));
    hipLaunchKernelGGL(k_sfd_load_target, dim3((unsigned)sfd_blocks_amp(n), n_targets), dim3(kSfdThreads), 0, st.h, d_t.p, src, dim,
                       n, O.target_little_endian);
    HIP_TRY(err, hipGetLastError());
  }

  S.B = batch, S.G = G, S.target_shared = target_shared ? 1 : 0, S.dim = dim, S.lo = lo.data();
  S.nblk_amp = sfd_blocks_amp(n), S.nblk_vec = sfd_blocks_vec(n);
  S.active = d_act.p, S.psi = d_psi.p, S.phi = d_phi.p, S.tgt = d_t.p, S.part_env = d_penv.p, S.part_ov = d_pov.p;
  SfdUpdateArgs& U = S.U;
  U.G = G, U.max_iter = max_iter, U.frozen = jit_frozen ? 1 : 0;
  U.beta1 = beta1, U.beta2 = beta2, U.eps = eps, U.tol = tol, U.param_tol = param_tol;
  U.lr_t = d_lr.p, U.env = d_env.p, U.ov = d_ov.p, U.gates = d_g.p, U.best = d_best.p, U.mom = d_m.p, U.vel = d_v.p;
  U.hist = d_hist.p, U.bv = d_bv.p, U.it = d_it.p, U.active = d_act.p;

  // the loop: check_every steps, then the stop flags
  float ms = 0.f;
  HIP_TRY(err, hipEventRecord(e0.h, st.h));
  HIP_TRY(err, hipStreamSynchronize(st.h));      // the uploads must not become part of the capture
  if (use_graph) S.capture(st.h);
  int* h_act = static_cast<int*>(pin.h);
  const long long most = sfd_max_steps_enqueued(max_iter, O.check_every);
  long long enq = 0;
  for (bool any = true; any && enq < most;) {
    for (int s = 0; s < O.check_every; ++s, ++enq) HIP_TRY(err, S.run(st.h));
    HIP_TRY(err, hipMemcpyAsync(h_act, d_act.p, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st.h));
    HIP_TRY(err, hipStreamSynchronize(st.h));
    any = false;
    for (int b = 0; b < batch; ++b) any |= h_act[b] != 0;
  }
  HIP_TRY(err, hipEventRecord(e1.h, st.h));
  HIP_TRY(err, hipStreamSynchronize(st.h));
  HIP_TRY(err, hipEventElapsedTime(&ms, e0.h, e1.h));
  if (total_ms) *total_ms = ms;
  if (steps_enqueued) *steps_enqueued = (int32_t)enq;

  // download
  HIP_TRY(err, download(opt_gates, d_best, gcount));
  HIP_TRY(err, download(final_gates, d_g, gcount));
  HIP_TRY(err, download(loss_history, d_hist, hcount));
  HIP_TRY(err, download(best_val, d_bv, batch));
  HIP_TRY(err, download(n_iter, d_it, batch));
  HIP_TRY(err, download(last_envs, d_env, gcount));
  HIP_TRY(err, download(last_overlap, d_ov, batch));
  return 0;
}
