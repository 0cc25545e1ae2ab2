// vqe_api.hip - host side of libvqe_hip.so: handle management, upload of the Hamiltonian layout (planned by
// ham_layout.h), batch upload and kernel dispatch behind the C ABI of include/vqe_hip.h.
#include "../../include/vqe_hip.h"
#include "vqe_device.h"
#include "vqe_devbuf.h"
#include "vqe_stream.h"
#include "vqe_dm.h"
#include "vqe_dm_batch.h"
#include "vqe_dm_grad.h"
#include "vqe_grad.h"
#include "vqe_lbfgs.h"
#include "vqe_spsa.h"
#include "vqe_stream_lbfgs.h"
#include "vqe_lanczos.h"
#include "vqe_qjump.h"
#include "vqe_stream_qjump.h"
#include "ham_layout.h"
#include "dm_host.h"
#include "env_step_host.h"
#include "noise_grad_host.h"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

using namespace vqe;

namespace {

std::string g_create_error;
}  // namespace

// The plan of one resident batch on the batched exact channel path (dm_host.h: DmBatchTables) on the device, with the
// matrices k_dm_build fills; made for the batch / noise setting of handle generation `gen`.
struct DmPlanSlot {
  uint64_t gen = ~0ull;
  DevBuf<int32_t> blk_begin, blk_circ, blk_win, mem_begin, mem;
  DevBuf<double> dep, S;
  std::vector<int32_t> h_blk_begin, h_mem_begin;
  int n_blocks = 0, max_blocks = 0;
  DmBatchDev dev{};
  // the adjoint gradient (vqe_dm_grad.h), made on the first gradient evaluation of the plan: the block of every member,
  // S^+ of every block, M of every block, the value of every member
  uint64_t grad_gen = ~0ull;
  DevBuf<int32_t> mem_blk;
  DevBuf<double> Sdag, M, val;
  int n_members = 0;
};

struct vqe_handle {
  int n = 0, dev = 0;
  bool lds_path = true;
  int cu_count = 0, lds_per_cu = 0, last_wg_per_cu = 0;
  // paired env-step launches (k_lds_minimize_pair): the switch (vqe_set_env_pairing) and what the last launch of an
  // LDS-resident kernel did (vqe_last_env_pairing)
  bool env_pairing = true;
  int last_pairs = 0, last_singles = 0;
  size_t last_lds = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float last_ms = 0.f;
  std::string err;

  DevBuf<double2> init;
  HamHost ham_host;   // Hamiltonian (host copy, grouped by X mask)
  int shard_rank = 0, shard_world = 1;
  int amp_rank = 0, amp_world = 1;
  bool ham_set = false;
  DevBuf<uint32_t> d_gx, d_term_z;
  DevBuf<double> d_term_cr, d_term_ci, d_tables;
  DevBuf<int32_t> d_tab_r, d_tab_i;

  DevBuf<int32_t> d_term_off;
  DevBuf<uint32_t> d_urec;   // unit path (HamDev::urec / uaddr / utab)
  DevBuf<uint32_t> d_uaddr;
  DevBuf<double> d_utab;
  HamDev ham{};
  double unit_score[4] = {1.0, 1.0, 1.0, 1.0};   // bank swizzle: mean / worst slot depth of the unit reads, identity then chosen
  NoiseCfg noise{0.0, 0.0, 0ull, 0ull, 0.0};
  // Pauli channels of the two noise slots (vqe_set_noise_pauli, noise_pauli.h): the weights as given, the
  // thresholds (host copy and the device buffer the samplers read), and the Kraus set of every slot that mode 1 and
  // the quantum-jump runs use - the override where one is installed, else the table's Pauli set, else none (channels)
  double pauli_w1[3] = {}, pauli_w2[15] = {};
  NoisePauliTab pauli_tab{};
  DevBuf<NoisePauliTab> d_pauli_tab;

  // single circuit
  std::vector<GateRec> circ;
  int circ_params = -1;

  // resident batch
  int batch = 0;
  int64_t total_params = 0;
  int max_ops = 0, max_params = 0, max_pair = 0;
  int max_rot = 0;       // most ops WITH a parameter in a circuit of the batch (rows of the noisy adjoint kernels' gacc)
  std::vector<int64_t> h_par_begin;
  std::vector<int32_t> h_par_count;
  DevBuf<GateRec> d_gates;
  DevBuf<int64_t> d_gate_begin, d_par_begin, d_scratch_begin;
  DevBuf<int32_t> d_gate_count, d_par_count, d_nfev, d_new_gate, d_order;
  bool has_new_gate = false;
  std::vector<int32_t> h_gate_count;
  // host copy of the resident batch (the streaming path builds the pre-action circuits of an env-step from it)
  std::vector<GateRec> h_gates;
  std::vector<int64_t> h_gate_begin;
  std::vector<double> h_theta;
  std::vector<int32_t> h_new_gate;
  // streaming env-step: the pre-action batch (device)
  DevBuf<GateRec> d_gates2;
  DevBuf<int64_t> d_gate_begin2, d_par_begin2;
  DevBuf<int32_t> d_gate_count2, d_par_count2;
  DevBuf<double> d_theta, d_x, d_xraw, d_f, d_scratch;
  DevBuf<double2> d_state;
  DevBuf<unsigned long long> d_dbg;
  DevBuf<double> d_trace;
  bool trace_on = false;
  int trace_maxfun = 0, trace_stride = 0, trace_batch = 0;
  // exact channel mode of the noisy path (vqe_set_noise_mode, vqe_dm.h): density matrix and its Hamiltonian terms
  int noise_mode = 0;
  DevBuf<double2> dm_rho;
  DevBuf<double> dm_S, dm_partial, dm_cr, dm_ci;
  DevBuf<uint32_t> dm_gx, dm_tz;
  DevBuf<int32_t> dm_toff;
  int dm_groups = 0, dm_blocks_last = 0;
  float dm_gpu_ms = 0.f;       // device time of the last exact-mode run (init + block sweeps + tr(rho H)), summed over its evaluations
  bool last_run_dm = false;
  hipEvent_t dm_ev0 = nullptr, dm_ev1 = nullptr;
  uint64_t dm_ham_gen = ~0ull;
  // batched lock-step form of the exact channel mode (vqe_set_dm_batched, vqe_dm_batch.h): the resident density matrices
  // of a chunk, the partials of their energies, the plans of the resident batch and of an env-step's pre-action batch
  int dm_batched = 0;          // max_resident: 0 serial path, -1 a quarter of the free memory, R >= 1
  size_t dm_auto_cap = 0;      // -1: the density matrices that fit, fixed at the first batched run
  int64_t dm_info[4] = {0, 0, 0, 0};
  DevBufExact<double2> dmb_rho;
  DevBuf<double> dmb_partial;
  DmPlanSlot dmb_full, dmb_pre;
  // adjoint gradient of that path (vqe_set_dm_grad, vqe_dm_grad.h): opt-in; the partial sums of M of a chunk's level
  bool dm_grad = false;
  // Kraus sets in the two channel slots (vqe_set_noise_kraus) and RXX / RYY / RZZ as members (vqe_set_dm_rot2), DESIGN
  // 4.16: both are part of what a plan is made for, so setting either bumps `gen`
  DmKraus kraus;
  DmKraus channels;      // (set_channels: made again by vqe_set_noise_kraus and vqe_set_noise_pauli)
  bool dm_rot2 = false;
  DevBuf<double> dmg_part;
  DevBuf<int32_t> dmg_active;
  // the lock-step driver of the device optimisers (lockstep_run): results of the circuits that stopped, the count of
  // running circuits; COBYLA's start points and per-circuit running flags
  DevBuf<double> ls_xres, ls_fres;
  DevBuf<int32_t> ls_nfres, ls_running;
  DevBuf<double> d_cob_x0;
  DevBuf<int32_t> d_cob_active;
  void* comm = nullptr;      // RCCL communicator of vqe_comm_init (ncclComm_t)
  int comm_world = 0;
  StreamWork sw;  // streaming-path work buffers
  uint64_t gen = 0;   // bumped whenever a resident batch / Hamiltonian shard / noise setting changes (plans of vqe_tile.h)
  // adjoint gradient (vqe_grad.h): unit-free table set of this handle's shard, built on the first gradient request
  uint64_t ham_ver = 0, grad_ham_ver = ~0ull;
  DevBuf<uint32_t> g_gx;
  DevBuf<int64_t> g_off;
  DevBuf<int32_t> g_cplx;
  DevBuf<double> g_tab, d_grad;
  DevBuf<double2> g_lam;
  GradHam gham{};
  // device L-BFGS (vqe_lbfgs.h): per-workgroup slices of the optimiser's vectors, per-circuit iteration count and status
  DevBuf<double> lb_work;
  DevBuf<int32_t> lb_nit, lb_status;
  int lb_batch = 0;      // circuits of the last L-BFGS run on the resident batch (0: none)
  // device Adam-SPSA (vqe_spsa.h): per-workgroup slices of x, m, v and the trial point; the options of the run
  DevBuf<double> spsa_work;
  DevBuf<SpsaOpts> spsa_opts;
  // adjoint gradient of the streaming path (vqe_stream_grad.h): opt-in (vqe_set_stream_grad); its backward sweep undoes
  // the circuit in place, so the states it leaves are not those a reduction-only launch may take
  bool stream_grad = false, stream_states_undone = false;
  // device L-BFGS of the streaming path (vqe_stream_lbfgs.h): opt-in (vqe_set_stream_lbfgs); per-stream records
  bool stream_lbfgs = false;
  DevBufExact<StreamLbfgsRec> lb_rec;
  // quantum-jump trajectories of a Kraus override in mode 0 (vqe_set_kraus_traj, vqe_qjump.h): the count (0: refused as
  // before), the channel tables of the two slots (made again when the override or p1 / p2 change: qj_ver), per-trajectory
  // energies and jump counts of the last evaluation, per-circuit jump sums
  // gradients of frozen Pauli-noise realisations in mode 0 (vqe_set_noise_grad): T (0: refused as before)
  // and whether a gradient run leaves eval_base where it is (a host optimiser's one deterministic function)
  int noise_grad_T = 0;
  bool noise_grad_hold = false;
  // ... on the streaming path (vqe_set_stream_noise_grad): max_resident (0: refused as before, -1 a quarter
  // of the free memory, R >= 1), the (circuit, realisation) pairs that fit (fixed at the first run), the expanded batch
  // and per-pair results, {max_resident, resident pairs, chunks, 0} of the last served run
  int sng_resident = 0;
  size_t sng_auto_cap = 0;
  int64_t sng_info[4] = {0, 0, 0, 0};
  StreamNoiseWork snw;
  int kraus_traj = 0;
  uint64_t qj_ver = 0, qj_tab_ver = ~0ull;
  DevBuf<double> qj_K1, qj_W1, qj_K2, qj_W2, qj_e;
  DevBuf<int32_t> qj_jumps;
  DevBuf<long long> qj_jsum;
  int qj_n1 = 0, qj_n2 = 0;
  int64_t qj_info[4] = {0, 0, 0, 0};
  int qj_traj_batch = 0;       // circuits whose per-trajectory energies vqe_batch_fetch_traj hands out (0: none)
  int qj_jsum_batch = 0;       // circuits of the last evaluation (its jump sums wait in qj_jsum)
  // ... on the streaming path (vqe_set_stream_kraus_traj, vqe_stream_qjump.h): max_resident (0: refused as before, -1 a
  // quarter of the free memory, R >= 1), the states that fit (fixed at the first run), the compiled circuits (records,
  // frame, jump positions, cos / sin), the partial rows and the matrix of the jump in flight of every resident state
  int sq_resident = 0;
  size_t sq_auto_cap = 0;
  int64_t sq_info[4] = {0, 0, 0, 0};
  DevBuf<QjOp> sq_ops;
  DevBuf<uint32_t> sq_masks;
  DevBuf<int32_t> sq_meta, sq_jpos;
  DevBuf<double2> sq_cs;
  DevBuf<double> sq_part, sq_kmat;
  // device Lanczos (vqe_lanczos.h): the solver's own copy of the full operator (logical frame) and its vectors
  LzWork lz;
};

#ifdef VQE_STAMPS
static unsigned long long cby_out_[8];
#endif
namespace {

int fail(vqe_t* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

template <class T>
int upload(vqe_t* h, DevBuf<T>& b, const T* src, size_t n) {
  HIP_TRY(h, b.reserve(n ? n : 1));
  if (n) HIP_TRY(h, hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return VQE_OK;
}
template <class T>
int upload(vqe_t* h, DevBuf<T>& b, const std::vector<T>& src) { return upload(h, b, src.data(), src.size()); }

// Build (or rebuild after re-sharding) the device Hamiltonian: plan the layout of shard (rank, world) of H - a new
// operator, or NULL for the one the handle holds - on the host (ham_layout.h), upload it.  A plan that fails leaves the
// handle as it was: host copy, shard numbers and generation counters change only once the plan stands, together.
int build_hamiltonian(vqe_t* h, HamHost* H, int rank, int world) {
  static const bool units_on = [] { const char* e = std::getenv("VQE_UNITS"); return !(e && e[0] == '0'); }();   // A/B knob
  HamLayout L;
  std::string err;
  if (!plan_hamiltonian(H ? *H : h->ham_host, h->n, h->lds_path, rank, world, units_on, L, err))
    return fail(h, VQE_EINVAL, err);
  if (H) h->ham_host = std::move(*H);
  h->shard_rank = rank;
  h->shard_world = world;
  h->ham_set = true;
  ++h->gen;
  ++h->ham_ver;
  VQE_TRY(upload(h, h->d_gx, L.gx));
  VQE_TRY(upload(h, h->d_tab_r, L.tab_r));
  VQE_TRY(upload(h, h->d_tab_i, L.tab_i));
  VQE_TRY(upload(h, h->d_tables, L.tables));
  VQE_TRY(upload(h, h->d_term_off, L.term_off));
  VQE_TRY(upload(h, h->d_term_z, L.term_z));
  VQE_TRY(upload(h, h->d_term_cr, L.term_cr));
  VQE_TRY(upload(h, h->d_term_ci, L.term_ci));
  const UnitArrays UA = unit_arrays(L, geo_lt(h->n));     // the units and the look-ahead trips behind them
  VQE_TRY(upload(h, h->d_urec, UA.urec));
  VQE_TRY(upload(h, h->d_uaddr, UA.uaddr));
  VQE_TRY(upload(h, h->d_utab, UA.utab));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // the layout goes out of scope
  HamDev& d = h->ham;
  d.n_groups = (int)L.gx.size();
  d.n_terms = (int)L.term_z.size();
  d.n_units = UA.n_units;
  d.gx = h->d_gx.p; d.tab_r = h->d_tab_r.p; d.tab_i = h->d_tab_i.p; d.tables = h->d_tables.p;
  d.urec = h->d_urec.p; d.uaddr = h->d_uaddr.p; d.utab = h->d_utab.p;
  d.term_off = h->d_term_off.p; d.term_z = h->d_term_z.p; d.term_cr = h->d_term_cr.p; d.term_ci = h->d_term_ci.p;
  d.has_diag = L.has_diag; d.n_real = L.n_real; d.n_cls = L.n_cls;
  std::copy(L.mrow, L.mrow + 16, d.mrow);
  d.swz = L.swz;
  h->unit_score[0] = L.mean0; h->unit_score[1] = L.worst0; h->unit_score[2] = L.mean; h->unit_score[3] = L.worst;
  return VQE_OK;
}

int check_gates(vqe_t* h, int64_t n_gates, const int32_t* kind, const int32_t* q0,
                const int32_t* q1, const int32_t* pidx, int n_params) {
  for (int64_t i = 0; i < n_gates; ++i) {
    const int k = kind[i];
    if (k < 0 || k > VQE_GATE_RZZ) return fail(h, VQE_EINVAL, "unknown gate kind");
    if (q0[i] < 0 || q0[i] >= h->n) return fail(h, VQE_EINVAL, "gate qubit out of range");
    if (k == VQE_GATE_CNOT || k == VQE_GATE_DEPOL2 || gate_is_rot2(k)) {
      if (q1[i] < 0 || q1[i] >= h->n || q1[i] == q0[i])
        return fail(h, VQE_EINVAL, "two-qubit gate needs two distinct qubits in range");
    }
    if (gate_is_rot(k)) {
      if (pidx[i] < 0 || pidx[i] >= n_params)
        return fail(h, VQE_EINVAL, "rotation parameter index out of range");
    }
  }
  return VQE_OK;
}

// What one run() does with the resident batch (EnvStep: Minimize on the pre-action circuits, float32 round trip, energy
// of the full circuits; Reduce: the streaming path's Pauli-term reduction alone, on the states of the previous run).
enum class Run { Energy, Minimize, State, EnvStep, Reduce };

// the optimiser kernels, told to follow CircuitEnv.step
void set_env_step(const vqe_t* h, BatchArgs& A) {
  A.env_step = 1;
  A.new_gate = h->has_new_gate ? h->d_new_gate.p : nullptr;
}

// The sizes of the LDS-resident kernels (kernel experiments, tools/build_only_n.sh: one size, seconds to build), and
// h->n as a compile-time N among them: f(std::integral_constant<int, N>), or the caller's refusal for any other n.
// (A left fold: the compiler then instantiates the kernels, and lays them out in the code object, in ascending N.)
#ifdef VQE_ONLY_N
using LdsSizes = std::integer_sequence<int, VQE_ONLY_N>;
#else
using LdsSizes = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13>;
#endif
template <class F, int... Ns>
int dispatch_n(vqe_t* h, const char* refusal, F f, std::integer_sequence<int, Ns...>) {
  int rc = 0;
  const bool found = (... || (h->n == Ns && ((rc = f(std::integral_constant<int, Ns>{})), true)));
  return found ? rc : fail(h, VQE_EINVAL, refusal);
}

// More than 64 parameters in a circuit (the trainable regime): the WIDE variant of the minimiser - on 256-thread
// workgroups the optimiser update runs on the whole workgroup (BlockCtx), on one-wave workgroups (n <= 9) the lanes
// walk their rows of the matrices side by side (WaveRowsCtx).  The plain variant keeps neither (registers).
constexpr int kWideMinN = 6;      // sizes below have no WIDE instantiation
bool wide_launch(int n, int max_params) {
  static const bool wide_on = [] { const char* e = std::getenv("VQE_WIDE_UPDATE"); return !(e && e[0] == '0'); }();   // A/B knob
  return n >= kWideMinN && wide_on && max_params > 64;
}

// vqe_cobyla_placement / vqe_batch_cobyla_placement: what a minimiser launch with these sizes does with a circuit of
// nvar variables (cobyla_placement of vqe_device.h - the function StagedCobyla::init calls - and the launcher's own
// size formulas).
// Why launch_lds refuses a batch of these sizes (lds: its dynamic LDS bytes), or nullptr
const char* lds_launch_refusal(int n, size_t lds, int max_ops, size_t lds_per_cu) {
  if (lds > lds_per_cu) return "circuit too large for the LDS-resident path (gates + parameters)";
  // register path: the raw ops are staged in the (idle) state region, 2^n records at most
  if (n >= kRegMinQubits && (size_t)max_ops > ((size_t)1 << n))
    return "circuit too large for the LDS-resident path (more than 2^n rotations)";
  return nullptr;
}

void report_placement(int n, int max_ops, int max_pair, int max_params, int n_groups, int nvar, bool wide, size_t lds_per_cu,
                      int64_t out[8]) {
  const bool resident = cobyla_resident_bytes(n, max_ops, max_params, n_groups, max_pair) != 0;
  const CobPlacement p = cobyla_placement(n, wide, resident, nvar);
  const size_t lds = lds_bytes(n, max_ops, max_params, n_groups, max_pair, wide);
  out[0] = p.resident ? VQE_COBYLA_RESIDENT : p.staged ? VQE_COBYLA_STAGED : p.block ? VQE_COBYLA_BLOCK
           : p.rows ? VQE_COBYLA_ROWS : VQE_COBYLA_GLOBAL;
  out[1] = p.pad;
  out[2] = p.words;
  out[3] = (int64_t)lds;
  out[4] = p.split;
  out[5] = (int64_t)cobyla_tile_bytes(n, max_params, wide);
  out[6] = (int64_t)cobyla_resident_bytes(n, max_ops, max_params, n_groups, max_pair);
  out[7] = lds_launch_refusal(n, lds, max_ops, lds_per_cu) == nullptr;
}

// Paired launch (k_lds_minimize_pair): how many workgroups of a batch carry two environments.  Pairing halves the
// rounds of workgroups a CU sees, and with them doubles the weight of the launch tail; single environments at the end
// of the LPT order could fill it, but measured they cost more than they give (4096 environments on 512 slots: 282.5 ms
// with none, 289.0 with 512, 286.6 with 1024; the episode's batches of 2048 likewise): every environment
// is paired, an odd one is left over.  VQE_PAIR_SINGLES=k sets k singles aside for such measurements.
constexpr int kPairMinMeanParams = 5;
int env_pair_count(int batch, int /*slots*/) {
  static const long singles = [] { const char* e = std::getenv("VQE_PAIR_SINGLES"); return e ? std::atol(e) : 0L; }();   // measurement knob
  const int ns = (int)std::min<long>(std::max<long>(singles, 0), batch);
  return (batch - ns) / 2;
}

template <int N>
int launch_lds_pair(vqe_t* h, const BatchArgs& A, size_t lds, int n_pairs) {
  if constexpr (N >= 10 && N <= 13) {
    void (*const kernel)(BatchArgs, int) = k_lds_minimize_pair<N>;
    const void* fn = (const void*)kernel;
    HIP_TRY(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {   // the unit loop addresses the state region absolutely (unit_lds_read): the dynamic LDS must start at 0
      hipFuncAttributes fa;
      HIP_TRY(h, hipFuncGetAttributes(&fa, fn));
      if (fa.sharedSizeBytes != 0) return fail(h, VQE_ESTATE, "LDS-resident kernel was built with static LDS");
    }
    h->last_wg_per_cu = std::max(1, std::min(8, (int)(h->lds_per_cu / lds)));
    h->last_pairs = n_pairs;
    h->last_singles = A.batch - 2 * n_pairs;
    h->last_lds = lds;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    const dim3 grid(A.batch - n_pairs), block(Geo<N>::NT);
    hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, A, n_pairs);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    return VQE_OK;
  } else {
    return fail(h, VQE_ESTATE, "no paired kernel at this size");
  }
}

template <int N>
int launch_lds(vqe_t* h, Run mode, BatchArgs A) {
  if (mode == Run::EnvStep) set_env_step(h, A);
  const bool minimize = mode == Run::Minimize || mode == Run::EnvStep;
  constexpr bool kHasWide = N >= kWideMinN;
  const bool wide = minimize && wide_launch(N, A.max_params);
  size_t lds = lds_bytes(N, A.max_ops, A.max_params, A.ham.n_groups, A.max_pair, wide);
  // measurement knob: VQE_LDS_PAD=bytes of unused LDS per workgroup lowers the workgroups per CU
  static const long lds_pad = [] { const char* e = std::getenv("VQE_LDS_PAD"); return e ? std::atol(e) : 0L; }();
  if (lds_pad > 0) lds += (size_t)lds_pad;
  if (const char* why = lds_launch_refusal(N, lds, A.max_ops, (size_t)h->lds_per_cu)) return fail(h, VQE_EINVAL, why);
  const bool noisy = A.noise.p1 > 0.0 || A.noise.p2 > 0.0;
  h->last_pairs = h->last_singles = 0;
  h->last_lds = lds;
  constexpr bool kW = false;     // up to 64 parameters per circuit: the instantiation without the workgroup-wide update
  void (*const kernel)(BatchArgs) =
      mode == Run::Energy ? k_lds_energy<N>
      : !minimize ? k_lds_state<N>
      : wide ? (noisy ? k_lds_minimize<N, kHasWide, true> : k_lds_minimize<N, kHasWide, false>)
             : (noisy ? k_lds_minimize<N, kW, true> : k_lds_minimize<N, kW, false>);
  const void* fn = (const void*)kernel;
  HIP_TRY(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  {   // the unit loop addresses the state region absolutely (unit_lds_read): the dynamic LDS must start at 0
    hipFuncAttributes fa;
    HIP_TRY(h, hipFuncGetAttributes(&fa, fn));
    if (fa.sharedSizeBytes != 0) return fail(h, VQE_ESTATE, "LDS-resident kernel was built with static LDS");
  }
  // Two environments per workgroup: the plain noiseless minimiser on four-wave workgroups, and only where the larger
  // LDS footprint leaves the workgroups per CU what they are (registers and LDS together: the runtime's own count)
  static const bool pair_on = [] { const char* e = std::getenv("VQE_ENV_PAIRING"); return !(e && e[0] == '0'); }();   // A/B knob
  if constexpr (N >= 10) {
    // ... and from kPairMinMeanParams variables per environment on average: below, the optimiser step is shorter than what
    // a round of the paired kernel spends on reloading an environment's scalars (measured, DESIGN 4.1: +4 % at a mean
    // of 4 variables, -10 % at 6)
    if (minimize && pair_on && h->env_pairing && !noisy && !wide && A.trace == nullptr && A.noise.shot_sigma == 0.0 &&
        lds_pad <= 0 && A.batch >= 1 && h->total_params >= (int64_t)kPairMinMeanParams * A.batch) {
      const size_t plds = pair_lds_plan(N, A.max_ops, A.max_params, A.ham.n_groups, A.max_pair).bytes;
      int occ_single = 0, occ_pair = -1;
      if (plds <= (size_t)h->lds_per_cu) {
        HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_single, fn, Geo<N>::NT, lds));
        void (*const pk)(BatchArgs, int) = k_lds_minimize_pair<N>;
        HIP_TRY(h, hipFuncSetAttribute((const void*)pk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plds));
        HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_pair, (const void*)pk, Geo<N>::NT, plds));
      }
      if (occ_pair == occ_single && occ_pair > 0) {
        const int n_pairs = env_pair_count(A.batch, occ_pair * h->cu_count);
        if (n_pairs > 0 || A.batch == 1) return launch_lds_pair<N>(h, A, plds, n_pairs);
      }
    }
  }
  h->last_wg_per_cu = std::max(1, std::min(8, (int)(h->lds_per_cu / lds)));
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  const dim3 grid(mode == Run::State ? 1 : A.batch), block(Geo<N>::NT);
  hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, A);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  return VQE_OK;
}

int dispatch_lds(vqe_t* h, Run mode, const BatchArgs& A) {
  return dispatch_n(h, "n_qubits outside the LDS-resident range",
                    [&](auto n) -> int { return launch_lds<decltype(n)::value>(h, mode, A); }, LdsSizes{});
}

// The noise setting a launch reads: p1 / p2 of vqe_set_noise, or for a slot with a table (vqe_set_noise_pauli) the
// table's total, and the address of the thresholds.  The handle's own p1 / p2 stay what vqe_set_noise made them.
NoiseCfg launch_noise(const vqe_t* h) {
  NoiseCfg nz = h->noise;
  if (h->pauli_tab.has1) nz.p1 = h->pauli_tab.cum1[2];
  if (h->pauli_tab.has2) nz.p2 = h->pauli_tab.cum2[14];
  nz.pauli = (h->pauli_tab.has1 || h->pauli_tab.has2) ? h->d_pauli_tab.p : nullptr;
  return nz;
}
// Pauli errors are drawn in mode 0 (by either rule)
bool pauli_noise_on(const vqe_t* h) {
  const NoiseCfg nz = launch_noise(h);
  return nz.p1 > 0.0 || nz.p2 > 0.0;
}
// The Kraus set of each slot for mode 1 and the quantum-jump runs: the override, else the table's Pauli set, else none
void set_channels(vqe_t* h) {
  h->channels = h->kraus;
  if (h->kraus.n1 == 0 && h->pauli_tab.has1) { pauli_kraus(h->pauli_w1, 2, h->channels.K1); h->channels.n1 = 4; }
  if (h->kraus.n2 == 0 && h->pauli_tab.has2) { pauli_kraus(h->pauli_w2, 4, h->channels.K2); h->channels.n2 = 16; }
}

BatchArgs make_args(vqe_t* h) {
  BatchArgs A{};
  A.n = h->n;
  A.batch = h->batch;
  A.gates = h->d_gates.p;
  A.gate_begin = h->d_gate_begin.p;
  A.gate_count = h->d_gate_count.p;
  A.par_begin = h->d_par_begin.p;
  A.par_count = h->d_par_count.p;
  A.order = h->d_order.p;
  A.theta = h->d_theta.p;
  A.xout = h->d_x.p;
  A.xraw = h->d_xraw.p;
  A.new_gate = nullptr;
  A.env_step = 0;
  A.fout = h->d_f.p;
  A.nfev = h->d_nfev.p;
  A.scratch = h->d_scratch.p;
  A.scratch_begin = h->d_scratch_begin.p;
  A.init = h->init.p;
  A.ham = h->ham;
  A.noise = launch_noise(h);
  A.max_ops = h->max_ops;
  A.max_pair = h->max_pair;
  A.max_params = h->max_params;
  A.state_out = h->d_state.p;
  A.dbg = h->d_dbg.p;
  A.trace = nullptr;
  A.amp_rank = h->amp_rank;
  A.amp_world = h->amp_world;
  return A;
}

// Load a batch given begin/count arrays (circuits may alias the same gate range).
int load_batch(vqe_t* h, int batch, const std::vector<GateRec>& gates,
               const std::vector<int64_t>& gbeg, const std::vector<int32_t>& gcnt,
               const std::vector<int64_t>& pbeg, const std::vector<int32_t>& pcnt,
               const double* theta0, int64_t total_params) {
  std::vector<int64_t> sbeg(batch);
  int64_t stot = 0;
  int max_ops = 1, max_par = 1, max_pair = 0, max_rot = 1;
  std::vector<double> cost(batch);
  for (int b = 0; b < batch; ++b) {
    sbeg[b] = stot;
    // the larger of the device contexts' paddings, + 1: k_s_cobyla (one thread per stream, HostCtx) keeps the value told
    // last right behind its optimiser's arrays (words(), which bind() lays out as scratch_doubles_ld counts them)
    // The slot costs nothing: scratch_doubles(P, 16) = 2 nv^2 + 12 nv + 19 with nv a multiple of 16, so it is 3 mod 16
    // and the rounding below ends on the same multiple of 16 with and without the + 1.
    const size_t sdoubles = cby::scratch_doubles(pcnt[b], 16) + 1;
    assert(cby::scratch_doubles_ld(pcnt[b], 1, cby::lead_dim(pcnt[b])) + 1 <= sdoubles);
    assert(((sdoubles + 15) & ~(size_t)15) == ((sdoubles - 1 + 15) & ~(size_t)15));
    stot += (int64_t)sdoubles;
    stot = (stot + 15) & ~(int64_t)15;  // 128-byte alignment: rows of the optimiser's global arrays are whole sectors / lines
    max_par = std::max(max_par, (int)pcnt[b]);
    int ops = 0, pair = 0, rot = 0;
    for (int64_t i = gbeg[b]; i < gbeg[b] + gcnt[b]; ++i) {
      const int k = gates[i].kind;
      ops += (k == G_CNOT) ? 0 : (k == G_DEPOL2 ? 2 : 1);
      pair += (k == G_RX || k == G_RY || k == G_RXX || k == G_RYY) ? 1 : 0;
      rot += gate_is_rot(k) ? 1 : 0;
    }
    max_rot = std::max(max_rot, rot);
    max_ops = std::max(max_ops, ops);
    max_pair = std::max(max_pair, pair);
    // expected cycles of one evaluation of the fused kernel beyond the constant energy step:
    // ~1.3 k per simulated op, ~22 per squared parameter for the optimiser update
    double ca = 1300.0, cb = 22.0, cc = 0.0;
    if (const char* e = getenv("VQE_LPT_COEF")) sscanf(e, "%lf,%lf,%lf", &ca, &cb, &cc);   // experiments
    cost[b] = ca * ops + cb * (double)pcnt[b] * (double)pcnt[b] + cc * (double)pcnt[b];
  }
  // workgroup i runs circuit order[i], longest first: the hardware hands workgroups to free CU
  // slots in index order, so the short circuits fill the end of the launch
  std::vector<int32_t> order(batch);
  for (int b = 0; b < batch; ++b) order[b] = b;
  if (!getenv("VQE_NO_LPT"))   // experiments: launch in caller order
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return cost[x] > cost[y]; });
  VQE_TRY(upload(h, h->d_gates, gates));
  VQE_TRY(upload(h, h->d_gate_begin, gbeg));
  VQE_TRY(upload(h, h->d_gate_count, gcnt));
  VQE_TRY(upload(h, h->d_par_begin, pbeg));
  VQE_TRY(upload(h, h->d_par_count, pcnt));
  VQE_TRY(upload(h, h->d_order, order));
  VQE_TRY(upload(h, h->d_scratch_begin, sbeg));
  VQE_TRY(upload(h, h->d_theta, theta0, (size_t)total_params));
  HIP_TRY(h, h->d_scratch.reserve((size_t)stot + 2));
  HIP_TRY(h, h->d_x.reserve((size_t)total_params + 1));
  HIP_TRY(h, h->d_xraw.reserve((size_t)total_params + 1));
  HIP_TRY(h, h->d_f.reserve(batch));
  HIP_TRY(h, h->d_nfev.reserve(batch));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->batch = batch;
  h->total_params = total_params;
  h->max_ops = (max_ops + 3) & ~3;
  h->max_pair = std::min(h->max_ops, (max_pair + 3) & ~3);
  h->max_params = (max_par + 3) & ~3;
  h->max_rot = max_rot;
  h->h_par_begin = pbeg;
  h->h_par_count = pcnt;
  h->h_gate_count = gcnt;
  h->h_gates = gates;
  h->h_gate_begin = gbeg;
  h->h_theta.assign(theta0, theta0 + total_params);
  h->has_new_gate = false;
  h->lb_batch = 0;
  h->qj_traj_batch = 0;
  ++h->gen;
  return VQE_OK;
}

int load_single(vqe_t* h, int batch, const double* theta) {
  if (h->circ_params < 0) return fail(h, VQE_ESTATE, "vqe_set_circuit has not been called");
  const int P = h->circ_params;
  std::vector<int64_t> gbeg(batch, 0), pbeg(batch);
  std::vector<int32_t> gcnt(batch, (int32_t)h->circ.size()), pcnt(batch, P);
  for (int b = 0; b < batch; ++b) pbeg[b] = (int64_t)b * P;
  return load_batch(h, batch, h->circ, gbeg, gcnt, pbeg, pcnt, theta, (int64_t)batch * P);
}

int ready(vqe_t* h) {
  if (!h) return VQE_EINVAL;
  if (!h->ham_set) return fail(h, VQE_ESTATE, "vqe_set_hamiltonian_pauli has not been called");
  if (h->batch <= 0) return fail(h, VQE_ESTATE, "no circuits loaded");
  return VQE_OK;
}

// one streaming-path evaluation of the batch that A describes, on the handle's work buffers and stream
int evaluate(vqe_t* h, const BatchArgs& A, uint64_t eval_id, StreamWant what) {
  return stream_evaluate(h->sw, A, h->stream, eval_id, what, h->err, h->gen);
}

// an owned host COBYLA (vqe_cobyla_create; null when the allocation failed)
struct CobylaDestroy { void operator()(vqe_cobyla_t* c) const { vqe_cobyla_destroy(c); } };
using CobylaPtr = std::unique_ptr<vqe_cobyla_t, CobylaDestroy>;
CobylaPtr make_cobyla(int n, const double* x0, const BatchArgs& A) {
  vqe_cobyla_t* c = nullptr;
  (void)vqe_cobyla_create(n, x0, A.rhobeg, A.rhoend, A.maxfun, &c);
  return CobylaPtr(c);
}

// The round-2 host-driven COBYLA of the streaming path (VQE_STREAM_HOST_COBYLA=1, kept for A/B runs): trial points
// and energies travel per evaluation.  x: in x0, out the result (layout pbeg / pcnt); trial points travel through d_x.
int stream_cobyla_host(vqe_t* h, BatchArgs& A, const std::vector<int64_t>& pbeg, const std::vector<int32_t>& pcnt,
                       std::vector<double>& x, std::vector<double>& f, std::vector<int32_t>& nfev) {
  const int B = h->batch;
  std::vector<CobylaPtr> cob(B);
  for (int b = 0; b < B; ++b)
    if (!(cob[b] = make_cobyla(pcnt[b], x.data() + pbeg[b], A))) return fail(h, VQE_ENOMEM, "host COBYLA allocation failed");
  HIP_TRY(h, h->d_x.reserve(x.size() + 1));
  uint64_t it = 0;
  for (;;) {
    int active = 0;
    for (int b = 0; b < B; ++b) active += vqe_cobyla_ask(cob[b].get(), x.data() + pbeg[b]) == 1;
    if (!active) break;
    if (!x.empty())
      HIP_TRY(h, hipMemcpyAsync(h->d_x.p, x.data(), x.size() * 8, hipMemcpyHostToDevice, h->stream));
    A.theta = h->d_x.p;  // trial points live in the output buffer; x0 stays untouched
    VQE_TRY(evaluate(h, A, h->noise.eval_base + (++it), StreamWant::Both));
    HIP_TRY(h, hipMemcpyAsync(f.data(), h->d_f.p, (size_t)B * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int b = 0; b < B; ++b)
      if (vqe_cobyla_ask(cob[b].get(), nullptr) == 1) vqe_cobyla_tell(cob[b].get(), f[b]);
  }
  for (int b = 0; b < B; ++b) vqe_cobyla_result(cob[b].get(), x.data() + pbeg[b], &f[b], &nfev[b], nullptr);
  return VQE_OK;
}

// ---- the lock-step driver of the device optimisers ------------------------------------------------------------------
// The optimisers whose evaluation is a train of launches - COBYLA on the streaming path and in the batched exact channel
// mode (k_s_cobyla, one thread per circuit), L-BFGS on the streaming path (k_sl_step, one wavefront per circuit) - keep
// the state of every resident circuit on the device and run all circuits in lock-step: one batched evaluation of the
// trial points in d_x, the running count zeroed, one step kernel that tells every optimiser its value and leaves the next
// trial points in d_x.  The host only queues launches and looks at the number of running circuits every kStreamPoll
// iterations and at maxfun - no copy of trial points or energies and no synchronisation per evaluation.  A circuit that
// stops writes x, f and nfev to ls_xres / ls_fres / ls_nfres; its trial point stays where it is (the evaluations go on
// over all circuits).
constexpr int kStreamPoll = 8;

// The buffers of such a run, and its start points x in d_x, where A.theta points from here on.
int lockstep_begin(vqe_t* h, BatchArgs& A, const std::vector<double>& x) {
  const size_t PT = x.size();
  HIP_TRY(h, h->d_x.reserve(PT + 1));
  HIP_TRY(h, h->ls_xres.reserve(PT + 1));
  HIP_TRY(h, h->ls_fres.reserve(h->batch));
  HIP_TRY(h, h->ls_nfres.reserve(h->batch));
  HIP_TRY(h, h->ls_running.reserve(1));
  if (PT) HIP_TRY(h, hipMemcpyAsync(h->d_x.p, x.data(), PT * 8, hipMemcpyHostToDevice, h->stream));
  A.theta = h->d_x.p;
  return VQE_OK;
}

// The loop, after lockstep_begin.  eval(it): queue the it-th batched evaluation (it = 1, 2, ...); step(it): queue the
// kernel that takes it (its running count: ls_running).  optimiser: the name in the error message.  Out: x, f, nfev.
template <class Eval, class Step>
int lockstep_run(vqe_t* h, const char* optimiser, int maxfun, std::vector<double>& x, std::vector<double>& f,
                 std::vector<int32_t>& nfev, Eval eval, Step step) {
  const int B = h->batch;
  uint64_t it = 0;
  int32_t running = 1;
  while (running > 0) {
    VQE_TRY(eval(++it));
    HIP_TRY(h, hipMemsetAsync(h->ls_running.p, 0, 4, h->stream));
    step(it);
    if (it % kStreamPoll == 0 || it >= (uint64_t)maxfun) {
      HIP_TRY(h, hipMemcpyAsync(&running, h->ls_running.p, 4, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (it > (uint64_t)maxfun + kStreamPoll) return fail(h, VQE_ESTATE, std::string("device ") + optimiser + " did not terminate");
  }
  HIP_TRY(h, hipGetLastError());
  if (!x.empty()) HIP_TRY(h, hipMemcpyAsync(x.data(), h->ls_xres.p, x.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(f.data(), h->ls_fres.p, (size_t)B * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(nfev.data(), h->ls_nfres.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

// COBYLA of all resident circuits in lock-step: the form scipy.optimize.minimize(..., method='COBYLA')
// (environment_qulacs_TN_notin_agent.py:478) takes where an evaluation is a train of launches.  k_s_cobyla is the host
// build's arithmetic; its start() runs before the first evaluation, so it is queued here, ahead of the loop.
// A: the batch to optimise (its par_begin / par_count lay out x); x: in x0, out the result.
// eval(A, it, active): queue the it-th batched evaluation of the trial points A.theta into d_f; active[b] != 0 for the
// circuits whose optimiser waits for that value - an evaluation may skip the others (the batched exact channel mode does,
// the streaming path evaluates all of them).
template <class Eval>
int lockstep_cobyla(vqe_t* h, BatchArgs& A, std::vector<double>& x, std::vector<double>& f, std::vector<int32_t>& nfev, Eval eval) {
  const int B = h->batch;
  VQE_TRY(lockstep_begin(h, A, x));
  HIP_TRY(h, h->d_cob_active.reserve(B));
  VQE_TRY(upload(h, h->d_cob_x0, x));
  auto cobyla_step = [&](bool first) {      // start() from x0, or tell() of the evaluation just made
    const auto kernel = first ? k_s_cobyla<true> : k_s_cobyla<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, B, (const int64_t*)A.par_begin,
                       (const int32_t*)A.par_count, (const int64_t*)h->d_scratch_begin.p, h->d_scratch.p,
                       (const double*)h->d_cob_x0.p, h->d_x.p, (const double*)h->d_f.p, A.rhobeg, A.rhoend, A.maxfun,
                       h->d_cob_active.p, h->ls_running.p, h->ls_xres.p, h->ls_fres.p, h->ls_nfres.p);
  };
  HIP_TRY(h, hipMemsetAsync(h->ls_running.p, 0, 4, h->stream));
  cobyla_step(true);
  return lockstep_run(h, "COBYLA", A.maxfun, x, f, nfev,
                      [&](uint64_t it) { return eval(A, it, (const int32_t*)h->d_cob_active.p); },
                      [&](uint64_t) { cobyla_step(false); });
}

// The streaming path's COBYLA: every evaluation is stream_evaluate on all streams (VQE_STREAM_HOST_COBYLA=1: the
// round-2 host-driven loop, kept for A/B runs).  pbeg / pcnt: the host copies of A.par_begin / A.par_count.
int stream_cobyla(vqe_t* h, BatchArgs& A, const std::vector<int64_t>& pbeg, const std::vector<int32_t>& pcnt,
                  std::vector<double>& x, std::vector<double>& f, std::vector<int32_t>& nfev) {
  static const bool host_loop = [] { const char* e = std::getenv("VQE_STREAM_HOST_COBYLA"); return e && e[0] == '1'; }();
  if (host_loop) return stream_cobyla_host(h, A, pbeg, pcnt, x, f, nfev);
  return lockstep_cobyla(h, A, x, f, nfev, [h](const BatchArgs& a, uint64_t it, const int32_t*) {
    return evaluate(h, a, h->noise.eval_base + it, StreamWant::Both);
  });
}

// The pre-action circuits of a streaming env-step (pre_action, vqe_geo.h; built by env_step_host.h) as a second
// resident batch: gates, layout and start point on the host, the device copies in d_*2, and A2 pointed at them.
struct PreActionBatch {
  std::vector<GateRec> gates;
  std::vector<int64_t> gbeg, pbeg;
  std::vector<int32_t> gcnt, pcnt, hole;
  std::vector<double> x0;
};
int load_pre_action_batch(vqe_t* h, PreActionBatch& pre, BatchArgs& A2) {
  const int B = h->batch;
  pre.gbeg.resize(B); pre.pbeg.resize(B); pre.gcnt.resize(B); pre.pcnt.resize(B); pre.hole.resize(B);
  pre.gates.reserve(h->h_gates.size());
  for (int b = 0; b < B; ++b) {
    pre.gbeg[b] = (int64_t)pre.gates.size();
    pre.pbeg[b] = (int64_t)pre.x0.size();
    pre.hole[b] = pre_action_circuit(h->h_gates.data() + h->h_gate_begin[b], h->h_gate_count[b],
                                     h->has_new_gate ? h->h_new_gate[b] : -1, h->h_theta.data() + h->h_par_begin[b],
                                     h->h_par_count[b], pre.gates, pre.x0).hole;
    pre.gcnt[b] = (int32_t)((int64_t)pre.gates.size() - pre.gbeg[b]);
    pre.pcnt[b] = (int32_t)((int64_t)pre.x0.size() - pre.pbeg[b]);
  }
  ++h->gen;      // d_gates2 changes content: plans made for it are stale
  VQE_TRY(upload(h, h->d_gates2, pre.gates));
  VQE_TRY(upload(h, h->d_gate_begin2, pre.gbeg));
  VQE_TRY(upload(h, h->d_gate_count2, pre.gcnt));
  VQE_TRY(upload(h, h->d_par_begin2, pre.pbeg));
  VQE_TRY(upload(h, h->d_par_count2, pre.pcnt));
  A2.gates = h->d_gates2.p; A2.gate_begin = h->d_gate_begin2.p; A2.gate_count = h->d_gate_count2.p;
  A2.par_begin = h->d_par_begin2.p; A2.par_count = h->d_par_count2.p;
  return VQE_OK;
}

// The end of a streaming env-step: pre.x0 holds the optima of the pre-action circuits.  They are merged into the full
// parameter vectors (the new gate's angle keeps its theta0 value), raw to d_xraw and rounded to float32 to d_x, and the
// full circuits are evaluated at the rounded angles (f of the env-step, d_f); nfev goes to d_nfev.
// eval(A): queue the evaluation of the batch that A describes at A.theta into d_f.
template <class Eval>
int finish_env_step(vqe_t* h, BatchArgs& A, const PreActionBatch& pre, const std::vector<int32_t>& nfev, Eval eval) {
  const int B = h->batch;
  std::vector<double> xraw(h->h_theta), xr32(h->h_theta);
  for (int b = 0; b < B; ++b) {
    const int64_t p0 = h->h_par_begin[b];
    merge_optimum(h->h_theta.data() + p0, h->h_par_count[b], pre.hole[b], pre.x0.data() + pre.pbeg[b], true, xr32.data() + p0, xraw.data() + p0);
  }
  if (h->total_params) {
    HIP_TRY(h, hipMemcpyAsync(h->d_x.p, xr32.data(), xr32.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_xraw.p, xraw.data(), xraw.size() * 8, hipMemcpyHostToDevice, h->stream));
  }
  HIP_TRY(h, hipMemcpyAsync(h->d_nfev.p, nfev.data(), (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));      // host vectors stay alive until the copies are done
  A.theta = h->d_x.p;
  return eval(A);
}

// The result of an optimiser run where vqe_batch_fetch and vqe_batch_fetch_xopt read it: x to d_x, xraw (the point before
// an environment step's float32 rounding; x itself outside one) to d_xraw, f to d_f, nfev to d_nfev.  Blocking: the
// host vectors may go out of scope.
int publish_optimum(vqe_t* h, const std::vector<double>& x, const std::vector<double>& xraw, const std::vector<double>& f,
                    const std::vector<int32_t>& nfev) {
  if (h->total_params) {
    HIP_TRY(h, hipMemcpyAsync(h->d_x.p, x.data(), x.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_xraw.p, xraw.data(), xraw.size() * 8, hipMemcpyHostToDevice, h->stream));
  }
  HIP_TRY(h, hipMemcpyAsync(h->d_f.p, f.data(), (size_t)h->batch * 8, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_nfev.p, nfev.data(), (size_t)h->batch * 4, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

// Run::Minimize / Run::EnvStep of a lock-step optimiser.  Minimize: optimise the resident batch from theta0, publish.
// EnvStep, one CircuitEnv.step() per circuit (environment_qulacs_TN_notin_agent.py:283-291): optimise the PRE-action
// circuits (pre_action, vqe_geo.h; built by env_step_host.h), float32 round trip, then the full circuits.
// optimise(A2, pre, x, f, nfev): the optimiser run on the batch A2 from x (out: the result); pre: the pre-action batch
// that A2 describes, NULL for the resident batch itself.  full_eval(A): finish_env_step's evaluation.  nfev: out.
template <class Optimise, class FullEval>
int minimize_or_env_step(vqe_t* h, bool env_step, BatchArgs& A, std::vector<int32_t>& nfev, Optimise optimise, FullEval full_eval) {
  std::vector<double> f(h->batch, 0.0);
  nfev.assign(h->batch, 0);
  if (!env_step) {
    std::vector<double> x(h->h_theta);
    VQE_TRY(optimise(A, (const PreActionBatch*)nullptr, x, f, nfev));
    return publish_optimum(h, x, x, f, nfev);
  }
  PreActionBatch pre;
  BatchArgs A2 = A;
  VQE_TRY(load_pre_action_batch(h, pre, A2));
  VQE_TRY(optimise(A2, (const PreActionBatch*)&pre, pre.x0, f, nfev));
  return finish_env_step(h, A, pre, nfev, full_eval);
}

// Streaming path (n >= 14): kernels per op; the COBYLA loop runs all streams in lock-step (one batched
// evaluation per iteration), its state on the device (stream_cobyla).
int stream_run(vqe_t* h, Run mode, BatchArgs& A) {
  if (mode == Run::Reduce && h->stream_states_undone)
    return fail(h, VQE_ESTATE, "the states of the last run were undone by its gradient sweep: run the energy first");
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  int rc = 0;
  if (mode != Run::Reduce) h->stream_states_undone = false;
  if (mode == Run::Energy) {
    rc = evaluate(h, A, h->noise.eval_base, StreamWant::Both);
  } else if (mode == Run::Reduce) {   // Pauli-term reduction only, on the states of the previous run
    if (h->sw.states.cap < ((size_t)h->batch << h->n)) return fail(h, VQE_ESTATE, "no states: run the energy first");
    rc = evaluate(h, A, h->noise.eval_base, StreamWant::Energy);
  } else if (mode == Run::State) {
    rc = evaluate(h, A, h->noise.eval_base, StreamWant::Circuit);
    if (!rc) {
      const size_t dim = (size_t)1 << h->n;
      hipLaunchKernelGGL(k_s_state_out, dim3((unsigned)(dim / kThreads)), dim3(kThreads), 0, h->stream, A,
                         h->sw.states.p, h->sw.masks.p, h->sw.meta.p);
      HIP_TRY(h, hipGetLastError());
    }
  } else {      // Run::Minimize, Run::EnvStep
    std::vector<int32_t> nfev;
    rc = minimize_or_env_step(h, mode == Run::EnvStep, A, nfev,
        [h](BatchArgs& a, const PreActionBatch* pre, std::vector<double>& x, std::vector<double>& f, std::vector<int32_t>& nf) {
          return stream_cobyla(h, a, pre ? pre->pbeg : h->h_par_begin, pre ? pre->pcnt : h->h_par_count, x, f, nf);
        },
        [h](const BatchArgs& a) { return evaluate(h, a, h->noise.eval_base + (uint64_t)a.maxfun + 1, StreamWant::Both); });
  }
  if (rc) return rc;
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  return VQE_OK;
}

// ---- exact channel mode (vqe_dm.h; superoperator blocks: dm_host.h) ---------------------------------

// this handle's Hamiltonian terms (all of its share under term sharding) for k_dm_energy
int dm_prepare_ham(vqe_t* h) {
  if (h->dm_ham_gen == h->gen) return VQE_OK;
  const HamHost& H = h->ham_host;
  std::vector<uint32_t> gx, tz;
  std::vector<int32_t> toff{0};
  std::vector<double> cr, ci;
  for (int g : shard_groups(H, h->lds_path, h->shard_rank, h->shard_world)) {
    gx.push_back(H.gx_all[g]);
    for (int k : H.group_terms[g]) { tz.push_back((uint32_t)H.hz[k]); cr.push_back(H.hcr[k]); ci.push_back(H.hci[k]); }
    toff.push_back((int32_t)tz.size());
  }
  VQE_TRY(upload(h, h->dm_gx, gx));
  VQE_TRY(upload(h, h->dm_tz, tz));
  VQE_TRY(upload(h, h->dm_toff, toff));
  VQE_TRY(upload(h, h->dm_cr, cr));
  VQE_TRY(upload(h, h->dm_ci, ci));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->dm_groups = (int)gx.size();
  h->dm_ham_gen = h->gen;
  return VQE_OK;
}

// tr(rho H) of one circuit into *e_host (blocking)
int dm_energy_one(vqe_t* h, const GateRec* g, int G, const double* theta, double* e_host) {
  const int n = h->n;
  std::vector<DmBlockHost> blocks;
  dm_make_blocks(n, g, G, theta, h->noise.p1, h->noise.p2, blocks, h->channels.any() ? &h->channels : nullptr, h->dm_rot2);
  std::vector<double> S(blocks.size() * 512);
  for (size_t k = 0; k < blocks.size(); ++k)
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
      S[k * 512 + r * 16 + c] = blocks[k].S.m[r][c].real();
      S[k * 512 + 256 + r * 16 + c] = blocks[k].S.m[r][c].imag();
    }
  const size_t total = (size_t)1 << (2 * n);
  const int eb = (int)((((size_t)1 << n) + 255) / 256);
  HIP_TRY(h, h->dm_rho.reserve(total));
  HIP_TRY(h, h->dm_partial.reserve((size_t)eb + 1));
  VQE_TRY(upload(h, h->dm_S, S));
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)h->cu_count * 16);
  if (!h->dm_ev0) { HIP_TRY(h, hipEventCreate(&h->dm_ev0)); HIP_TRY(h, hipEventCreate(&h->dm_ev1)); }
  HIP_TRY(h, hipEventRecord(h->dm_ev0, h->stream));
  hipLaunchKernelGGL(k_dm_init, dim3(grid), dim3(256), 0, h->stream, h->dm_rho.p, (const double2*)h->init.p, n);
  for (size_t k = 0; k < blocks.size(); ++k) {
    DmBlockArgs A{};
    A.rho = h->dm_rho.p; A.S = h->dm_S.p + k * 512; A.n = n; A.a = blocks[k].a; A.b = blocks[k].b;
    int hb[4] = {A.a, A.b, A.a + n, A.b + n};
    std::sort(hb, hb + 4);
    for (int i = 0; i < 4; ++i) A.hole[i] = hb[i];
    A.n_groups = (uint32_t)(total / 16);
    const size_t tiles = (A.n_groups + 15) / 16;
    const unsigned gb = (unsigned)std::max<size_t>(1, std::min<size_t>((tiles + 3) / 4, (size_t)h->cu_count * 8));
    hipLaunchKernelGGL(k_dm_block, dim3(gb), dim3(256), 0, h->stream, A);
  }
  hipLaunchKernelGGL(k_dm_energy, dim3(eb), dim3(256), 0, h->stream, (const double2*)h->dm_rho.p, n, h->dm_groups,
                     (const uint32_t*)h->dm_gx.p, (const int32_t*)h->dm_toff.p, (const uint32_t*)h->dm_tz.p,
                     (const double*)h->dm_cr.p, (const double*)h->dm_ci.p, h->dm_partial.p);
  hipLaunchKernelGGL(k_dm_sum, dim3(1), dim3(64), 0, h->stream, (const double*)h->dm_partial.p, eb, h->dm_partial.p + eb);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(h->dm_ev1, h->stream));
  HIP_TRY(h, hipMemcpyAsync(e_host, h->dm_partial.p + eb, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));      // (S and the blocks go out of scope)
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->dm_ev0, h->dm_ev1));
  h->dm_gpu_ms += ms;
  h->dm_blocks_last = (int)blocks.size();
  return VQE_OK;
}

// ---- the batched lock-step form (vqe_set_dm_batched; kernels: vqe_dm_batch.h) --------

// The plan of the batch (gates, gbeg, gcnt) in slot P, made once per handle generation.
int dm_batch_plan(vqe_t* h, DmPlanSlot& P, const std::vector<GateRec>& gates, const std::vector<int64_t>& gbeg,
                  const std::vector<int32_t>& gcnt) {
  if (P.gen == h->gen) return VQE_OK;
  DmBatchTables T;
  dm_flatten_plans(h->n, h->batch, gates.data(), gbeg.data(), gcnt.data(), h->noise.p1, h->noise.p2, T,
                   h->channels.any() ? &h->channels : nullptr, h->dm_rot2);
  VQE_TRY(upload(h, P.blk_begin, T.blk_begin));
  VQE_TRY(upload(h, P.blk_circ, T.blk_circ));
  VQE_TRY(upload(h, P.blk_win, T.blk_win));
  VQE_TRY(upload(h, P.mem_begin, T.mem_begin));
  VQE_TRY(upload(h, P.mem, T.mem));
  VQE_TRY(upload(h, P.dep, T.dep));
  P.n_blocks = (int)T.blk_circ.size();
  P.max_blocks = T.max_blocks;
  HIP_TRY(h, P.S.reserve((size_t)std::max(1, P.n_blocks) * 512));
  HIP_TRY(h, hipStreamSynchronize(h->stream));      // the tables go out of scope
  P.h_blk_begin = std::move(T.blk_begin);
  P.h_mem_begin = std::move(T.mem_begin);
  P.dev =DmBatchDev{P.blk_begin.p, P.blk_circ.p, P.blk_win.p, P.mem_begin.p, P.mem.p, P.dep.p, P.S.p};
  P.gen = h->gen;
  return VQE_OK;
}

// The resident density matrices R of this run and their buffers; info[0], [1].
int dm_batch_reserve(vqe_t* h) {
  const size_t total = (size_t)1 << (2 * h->n);
  if (h->dm_batched < 0 && !h->dm_auto_cap) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    h->dm_auto_cap = std::max<size_t>(1, (free_b / 4) / (total * sizeof(double2)));
  }
  const size_t cap = h->dm_batched > 0 ? (size_t)h->dm_batched : h->dm_auto_cap;
  const int R = (int)std::min<size_t>(std::min<size_t>(cap, (size_t)h->batch), 65535);      // a chunk is the y extent of a grid
  const size_t eb = (((size_t)1 << h->n) + 255) / 256;
  HIP_TRY(h, h->dmb_rho.reserve((size_t)R * total));
  HIP_TRY(h, h->dmb_partial.reserve((size_t)R * eb));
  h->dm_info[0] = R;
  h->dm_info[1] = (h->batch + R - 1) / R;
  return VQE_OK;
}

// One lock-step evaluation: the circuits of plan P (the batch A describes) at A.theta, tr(rho H) into A.fout[b] for
// every active circuit.  Queued on the handle's stream; nothing is copied back.
int dm_batch_eval(vqe_t* h, const DmPlanSlot& P, const BatchArgs& A, const int32_t* active) {
  const int n = h->n, B = h->batch, R = (int)h->dm_info[0];
  const size_t total = (size_t)1 << (2 * n);
  const uint32_t n_groups = (uint32_t)(total / 16);
  const size_t tiles = ((size_t)n_groups + 15) / 16;
  const unsigned eb = (unsigned)((((size_t)1 << n) + 255) / 256);
  if (P.n_blocks)
    hipLaunchKernelGGL(k_dm_build, dim3((unsigned)P.n_blocks), dim3(256), 0, h->stream, P.dev, (const double*)A.theta,
                       (const int64_t*)A.par_begin, active);
  for (int c0 = 0; c0 < B; c0 += R) {
    const int cnt = std::min(R, B - c0);
    int levels = 0;
    for (int b = c0; b < c0 + cnt; ++b) levels = std::max(levels, P.h_blk_begin[b + 1] - P.h_blk_begin[b]);
    // workgroups per circuit: what the serial path launches for one circuit, shared out when the chunk fills the device
    const size_t share = (size_t)h->cu_count * 16 / (size_t)cnt;
    const unsigned gi = (unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, std::max<size_t>(8, share)));
    const unsigned gb = (unsigned)std::max<size_t>(1, std::min<size_t>((tiles + 3) / 4, std::max<size_t>(8, share / 2)));
    hipLaunchKernelGGL(k_dm_init_b, dim3(gi, (unsigned)cnt), dim3(256), 0, h->stream, h->dmb_rho.p, (const double2*)h->init.p, n, c0, active);
    for (int l = 0; l < levels; ++l)
      hipLaunchKernelGGL(k_dm_block_b, dim3(gb, (unsigned)cnt), dim3(256), 0, h->stream, h->dmb_rho.p, P.dev, n, n_groups, l, c0, active);
    hipLaunchKernelGGL(k_dm_energy_b, dim3(eb, (unsigned)cnt), dim3(256), 0, h->stream, (const double2*)h->dmb_rho.p, n, h->dm_groups,
                       (const uint32_t*)h->dm_gx.p, (const int32_t*)h->dm_toff.p, (const uint32_t*)h->dm_tz.p,
                       (const double*)h->dm_cr.p, (const double*)h->dm_ci.p, h->dmb_partial.p, c0, active);
    hipLaunchKernelGGL(k_dm_sum_b, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, h->stream, (const double*)h->dmb_partial.p, (int)eb,
                       cnt, c0, active, A.fout);
  }
  HIP_TRY(h, hipGetLastError());
  return VQE_OK;
}

// Run::Energy / Minimize / EnvStep of the batched path, in the shape of stream_run's branches: the optimiser of every
// circuit lives on the device (k_s_cobyla through lockstep_cobyla), an evaluation is dm_batch_eval.
int dm_run_batched(vqe_t* h, Run mode, BatchArgs A) {
  VQE_TRY(dm_batch_reserve(h));
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  int64_t evals = 1;
  if (mode == Run::Energy) {
    VQE_TRY(dm_batch_plan(h, h->dmb_full, h->h_gates, h->h_gate_begin, h->h_gate_count));
    VQE_TRY(dm_batch_eval(h, h->dmb_full, A, nullptr));
  } else {
    // Run::Minimize, Run::EnvStep: the pre-action circuits of an env-step are a second resident batch with a plan of its
    // own (dmb_pre); the plan of the full circuits is made before their evaluation
    const auto plan_full = [h] { return dm_batch_plan(h, h->dmb_full, h->h_gates, h->h_gate_begin, h->h_gate_count); };
    std::vector<int32_t> nfev;
    VQE_TRY(minimize_or_env_step(h, mode == Run::EnvStep, A, nfev,
        [&](BatchArgs& a, const PreActionBatch* pre, std::vector<double>& x, std::vector<double>& f, std::vector<int32_t>& nf) {
          DmPlanSlot& P = pre ? h->dmb_pre : h->dmb_full;
          VQE_TRY(pre ? dm_batch_plan(h, P, pre->gates, pre->gbeg, pre->gcnt) : plan_full());
          return lockstep_cobyla(h, a, x, f, nf, [h, &P](const BatchArgs& t, uint64_t, const int32_t* active) {
            return dm_batch_eval(h, P, t, active);
          });
        },
        [&](const BatchArgs& a) {
          VQE_TRY(plan_full());
          return dm_batch_eval(h, h->dmb_full, a, nullptr);
        }));
    evals = *std::max_element(nfev.begin(), nfev.end()) + (mode == Run::EnvStep ? 1 : 0);
  }
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  h->dm_info[2] = evals;
  h->dm_info[3] = h->dmb_full.max_blocks;
  h->dm_blocks_last = h->dmb_full.max_blocks;
  return VQE_OK;
}

// The resident batch in exact channel mode: Run::Energy, or COBYLA (host-driven on exact energies; Run::EnvStep: on the
// pre-action circuit, then float32 round trip and the energy of the full circuit, as the fused kernel does).  After
// vqe_set_dm_batched: dm_run_batched, behind the same refusals.
// What the exact channel mode cannot serve (checked by run(), before anything of the handle changes)
int dm_refusal(vqe_t* h) {
  if (h->n < 2 || h->n > 13) return fail(h, VQE_EINVAL, "the exact channel mode (density matrix) serves 2 <= n_qubits <= 13");
  // without vqe_set_dm_rot2 the superoperator blocks (dm_host.h) are built from CNOT, RX, RY, RZ and the two channels only:
  // refused before anything is launched
  for (int b = 0; !h->dm_rot2 && b < h->batch; ++b)
    for (int64_t i = h->h_gate_begin[b]; i < h->h_gate_begin[b] + h->h_gate_count[b]; ++i)
      if (gate_is_rot2(h->h_gates[i].kind))
        return fail(h, VQE_EINVAL, "the exact channel mode does not take RXX / RYY / RZZ gates (use Pauli-trajectory noise, vqe_set_noise_mode 0)");
  if (h->amp_world > 1) return fail(h, VQE_ESTATE, "the exact channel mode has no amplitude sharding");
  return VQE_OK;
}

int dm_run(vqe_t* h, Run mode, const BatchArgs& A) {
  VQE_TRY(dm_prepare_ham(h));
  std::fill(h->dm_info, h->dm_info + 4, (int64_t)0);
  if (h->dm_batched != 0) return dm_run_batched(h, mode, A);
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  h->dm_gpu_ms = 0.f;
  h->last_run_dm = true;
  const int B = h->batch;
  const bool env_step = mode == Run::EnvStep;
  std::vector<double> f(B, 0.0), x(h->h_theta), xraw(h->h_theta);
  std::vector<int32_t> nfev(B, 1);
  for (int b = 0; b < B; ++b) {
    const GateRec* g = h->h_gates.data() + h->h_gate_begin[b];
    const int G = h->h_gate_count[b], P = h->h_par_count[b];
    double* xb = x.data() + h->h_par_begin[b];
    if (mode == Run::Energy) {
      VQE_TRY(dm_energy_one(h, g, G, xb, &f[b]));
      continue;
    }
    // the circuit COBYLA sees: the pre-action circuit (pre_action, vqe_geo.h) when this is an env-step
    std::vector<GateRec> g2;
    std::vector<double> xo;
    const int hole = pre_action_circuit(g, G, (env_step && h->has_new_gate) ? h->h_new_gate[b] : -1, xb, P, g2, xo).hole;
    double fo = 0.0;
    if (xo.empty()) {      // scipy returns after one evaluation
      VQE_TRY(dm_energy_one(h, g2.data(), (int)g2.size(), xo.data(), &fo));
    } else {
      const CobylaPtr cob = make_cobyla((int)xo.size(), xo.data(), A);
      if (!cob) return fail(h, VQE_ENOMEM, "host COBYLA allocation failed");
      std::vector<double> xt(xo.size());
      while (vqe_cobyla_ask(cob.get(), xt.data()) == 1) {
        double e;
        VQE_TRY(dm_energy_one(h, g2.data(), (int)g2.size(), xt.data(), &e));
        vqe_cobyla_tell(cob.get(), e);
      }
      vqe_cobyla_result(cob.get(), xo.data(), &fo, &nfev[b], nullptr);
    }
    merge_optimum(h->h_theta.data() + h->h_par_begin[b], P, hole, xo.data(), env_step, xb, xraw.data() + h->h_par_begin[b]);
    f[b] = fo;
    if (env_step) VQE_TRY(dm_energy_one(h, g, G, xb, &f[b]));
  }
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  if (mode != Run::Energy) return publish_optimum(h, x, xraw, f, nfev);
  HIP_TRY(h, hipMemcpyAsync(h->d_f.p, f.data(), (size_t)B * 8, hipMemcpyHostToDevice, h->stream));      // (no optimum: x stays)
  HIP_TRY(h, hipMemcpyAsync(h->d_nfev.p, nfev.data(), (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

// ---- adjoint gradient and device L-BFGS of the batched form (vqe_set_dm_grad; kernels: vqe_dm_grad.h) ----

// The handle serves gradients in the exact channel mode: the mode, the switch and the batched path
bool dm_grad_path(const vqe_t* h) { return h->noise_mode == 1 && h->dm_grad && h->dm_batched != 0; }

// dm_refusal's gate test on the single circuit of vqe_set_circuit, for the calls that would load it as the batch:
// refused before the resident batch changes
int dm_circuit_refusal(vqe_t* h) {
  if (!dm_grad_path(h) || h->dm_rot2) return VQE_OK;
  for (const GateRec& g : h->circ)
    if (gate_is_rot2(g.kind))
      return fail(h, VQE_EINVAL, "the exact channel mode does not take RXX / RYY / RZZ gates (use Pauli-trajectory noise, vqe_set_noise_mode 0)");
  return VQE_OK;
}

// The gradient tables of plan P and the resident circuits R of a gradient run on it (dm_grad_resident: levels + 2
// density matrices per circuit out of the budget of an energy run), with their buffers; info[0], [1], [3].
int dm_grad_reserve(vqe_t* h, DmPlanSlot& P) {
  const int n = h->n;
  const size_t total = (size_t)1 << (2 * n);
  if (P.grad_gen != P.gen) {
    P.n_members = P.h_mem_begin.back();
    std::vector<int32_t> mem_blk((size_t)P.n_members);
    for (int k = 0; k < P.n_blocks; ++k)
      for (int m = P.h_mem_begin[k]; m < P.h_mem_begin[k + 1]; ++m) mem_blk[m] = k;
    VQE_TRY(upload(h, P.mem_blk, mem_blk));
    HIP_TRY(h, P.Sdag.reserve((size_t)std::max(1, P.n_blocks) * 512));
    HIP_TRY(h, P.M.reserve((size_t)std::max(1, P.n_blocks) * 512));
    HIP_TRY(h, P.val.reserve((size_t)std::max(1, P.n_members)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // mem_blk goes out of scope
    P.grad_gen = P.gen;
  }
  if (h->dm_batched < 0 && !h->dm_auto_cap) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    h->dm_auto_cap = std::max<size_t>(1, (free_b / 4) / (total * sizeof(double2)));
  }
  const size_t cap = h->dm_batched > 0 ? (size_t)h->dm_batched : h->dm_auto_cap;
  const int R = dm_grad_resident(cap * total * sizeof(double2), n, P.max_blocks, h->batch);
  if (R < 1)
    return fail(h, VQE_ENOMEM, "a gradient in the exact channel mode keeps levels + 2 = " + std::to_string(P.max_blocks + 2) +
                               " density matrices per resident circuit; the budget (vqe_set_dm_batched) holds " + std::to_string(cap));
  const size_t eb = (((size_t)1 << n) + 255) / 256;
  HIP_TRY(h, h->dmb_rho.reserve((size_t)R * ((size_t)P.max_blocks + 2) * total));
  HIP_TRY(h, h->dmb_partial.reserve((size_t)R * eb));
  HIP_TRY(h, h->dmg_part.reserve((size_t)R * dm_grad_partials(n) * 512));
  h->dm_info[0] = R;
  h->dm_info[1] = (h->batch + R - 1) / R;
  h->dm_info[3] = P.max_blocks;
  return VQE_OK;
}

// One lock-step gradient evaluation after dm_grad_reserve(h, P): the circuits of plan P (the batch A describes) at
// A.theta, tr(rho H) into A.fout[b] and dE/dtheta into d_grad (layout A.par_begin / A.par_count) for every active
// circuit.  Queued on the handle's stream; nothing is copied back.
int dm_grad_eval(vqe_t* h, const DmPlanSlot& P, const BatchArgs& A, const int32_t* active) {
  const int n = h->n, B = h->batch, R = (int)h->dm_info[0];
  const size_t total = (size_t)1 << (2 * n);
  const uint32_t n_groups = (uint32_t)(total / 16);
  const size_t tiles = ((size_t)n_groups + 15) / 16;
  const unsigned eb = (unsigned)((((size_t)1 << n) + 255) / 256);
  const uint32_t tpp = dm_grad_tiles_per_partial(n), n_part = dm_grad_partials(n);
  DmBatchDev Td = P.dev;      // the sweep of Lambda: the same blocks and windows, S^+ for S
  Td.S = P.Sdag.p;
  double2* const lam = h->dmb_rho.p;
  const auto state = [&](int level) { return h->dmb_rho.p + ((size_t)level + 1) * (size_t)R * total; };
  if (P.n_blocks) {
    hipLaunchKernelGGL(k_dm_build, dim3((unsigned)P.n_blocks), dim3(256), 0, h->stream, P.dev, (const double*)A.theta,
                       (const int64_t*)A.par_begin, active);
    hipLaunchKernelGGL(k_dmg_adjoint, dim3((unsigned)P.n_blocks), dim3(256), 0, h->stream, P.dev, P.Sdag.p, active);
  }
  for (int c0 = 0; c0 < B; c0 += R) {
    const int cnt = std::min(R, B - c0);
    int levels = 0;
    for (int b = c0; b < c0 + cnt; ++b) levels = std::max(levels, P.h_blk_begin[b + 1] - P.h_blk_begin[b]);
    const size_t share = (size_t)h->cu_count * 16 / (size_t)cnt;      // the grids of dm_batch_eval
    const unsigned gi = (unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, std::max<size_t>(8, share)));
    const unsigned gb = (unsigned)std::max<size_t>(1, std::min<size_t>((tiles + 3) / 4, std::max<size_t>(8, share / 2)));
    hipLaunchKernelGGL(k_dm_init_b, dim3(gi, (unsigned)cnt), dim3(256), 0, h->stream, state(0), (const double2*)h->init.p, n, c0, active);
    for (int l = 0; l < levels; ++l)
      hipLaunchKernelGGL(k_dmg_forward, dim3(gb, (unsigned)cnt), dim3(256), 0, h->stream, (const double2*)state(l), state(l + 1), P.dev, n,
                         n_groups, l, c0, active);
    hipLaunchKernelGGL(k_dm_energy_b, dim3(eb, (unsigned)cnt), dim3(256), 0, h->stream, (const double2*)state(levels), n, h->dm_groups,
                       (const uint32_t*)h->dm_gx.p, (const int32_t*)h->dm_toff.p, (const uint32_t*)h->dm_tz.p,
                       (const double*)h->dm_cr.p, (const double*)h->dm_ci.p, h->dmb_partial.p, c0, active);
    hipLaunchKernelGGL(k_dm_sum_b, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, h->stream, (const double*)h->dmb_partial.p, (int)eb,
                       cnt, c0, active, A.fout);
    hipLaunchKernelGGL(k_dmg_lambda_zero, dim3(gi, (unsigned)cnt), dim3(256), 0, h->stream, lam, n, c0, active);
    hipLaunchKernelGGL(k_dmg_lambda_set, dim3(eb, (unsigned)cnt), dim3(256), 0, h->stream, lam, n, h->dm_groups,
                       (const uint32_t*)h->dm_gx.p, (const int32_t*)h->dm_toff.p, (const uint32_t*)h->dm_tz.p,
                       (const double*)h->dm_cr.p, (const double*)h->dm_ci.p, c0, active);
    for (int l = levels - 1; l >= 0; --l) {      // block index l = level l + 1 of the mathematics: rho_l beside Lambda_{l+1}
      hipLaunchKernelGGL(k_dmg_macc, dim3((n_part + 3) / 4, (unsigned)cnt), dim3(256), 0, h->stream, (const double2*)state(l),
                         (const double2*)lam, P.dev, n, n_groups, tpp, n_part, l, c0, active, h->dmg_part.p);
      hipLaunchKernelGGL(k_dmg_msum, dim3((unsigned)cnt), dim3(512), 0, h->stream, (const double*)h->dmg_part.p, P.dev, n_part, l, c0,
                         active, P.M.p);
      hipLaunchKernelGGL(k_dm_block_b, dim3(gb, (unsigned)cnt), dim3(256), 0, h->stream, lam, Td, n, n_groups, l, c0, active);
    }
  }
  if (P.n_members)
    hipLaunchKernelGGL(k_dmg_contract, dim3((unsigned)P.n_members), dim3(256), 0, h->stream, P.dev, (const int32_t*)P.mem_blk.p,
                       (const double*)A.theta, (const int64_t*)A.par_begin, active, (const double*)P.M.p, P.val.p);
  hipLaunchKernelGGL(k_dmg_scatter, dim3((unsigned)B), dim3(64), 0, h->stream, P.dev, (const int64_t*)A.par_begin,
                     (const int32_t*)A.par_count, active, (const double*)P.val.p, h->d_grad.p);
  HIP_TRY(h, hipGetLastError());
  return VQE_OK;
}

// run_grad in the exact channel mode: E into d_f, the gradient into d_grad.
int dm_run_grad(vqe_t* h) {
  VQE_TRY(dm_refusal(h));
  HIP_TRY(h, hipSetDevice(h->dev));
  VQE_TRY(dm_prepare_ham(h));
  VQE_TRY(dm_batch_plan(h, h->dmb_full, h->h_gates, h->h_gate_begin, h->h_gate_count));
  int64_t info[4];
  std::copy(h->dm_info, h->dm_info + 4, info);
  if (const int rc = dm_grad_reserve(h, h->dmb_full)) {      // refused: the handle as it was
    std::copy(info, info + 4, h->dm_info);
    return rc;
  }
  HIP_TRY(h, h->d_grad.reserve((size_t)h->total_params + 1));
  const BatchArgs A = make_args(h);
  h->last_run_dm = false;
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  VQE_TRY(dm_grad_eval(h, h->dmb_full, A, nullptr));
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  h->dm_info[2] = 1;
  h->dm_blocks_last = h->dmb_full.max_blocks;
  return VQE_OK;
}

// The device L-BFGS of the resident circuits in lock-step, stream_lbfgs with dm_grad_eval as the evaluation: k_sl_step
// keeps its running flags in its records, k_dmg_active hands them to the evaluation kernels as their `active` array, so
// a circuit that has stopped costs an early exit per workgroup.
int dm_lbfgs(vqe_t* h, const DmPlanSlot& P, BatchArgs& A, const vqe_lbfgs_opts_t& o, std::vector<double>& x, std::vector<double>& f,
             std::vector<int32_t>& nfev) {
  const int B = h->batch;
  HIP_TRY(h, h->d_grad.reserve(x.size() + 1));
  HIP_TRY(h, h->lb_work.reserve((size_t)B * lbfgs_work_doubles(A.max_params, o.history)));
  HIP_TRY(h, h->lb_nit.reserve(B));
  HIP_TRY(h, h->lb_status.reserve(B));
  HIP_TRY(h, h->lb_rec.reserve(B));
  HIP_TRY(h, h->dmg_active.reserve(B));
  VQE_TRY(lockstep_begin(h, A, x));
  const StreamLbfgsArgs T{A.par_begin, A.par_count, A.max_params, h->lb_rec.p, h->d_x.p, h->d_f.p, h->d_grad.p,
                          h->ls_running.p, h->ls_xres.p, h->ls_fres.p, h->ls_nfres.p};
  const LbfgsArgs O{o.history, o.maxiter, o.maxfun, o.max_ls, o.gtol, o.ftol, o.c1, h->lb_work.p, h->lb_nit.p, h->lb_status.p};
  return lockstep_run(h, "L-BFGS", o.maxfun, x, f, nfev,
                      [&](uint64_t it) {
                        if (it == 1) return dm_grad_eval(h, P, A, nullptr);
                        hipLaunchKernelGGL(k_dmg_active, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream,
                                           (const int32_t*)&h->lb_rec.p->active, (int)(sizeof(StreamLbfgsRec) / 4), B, h->dmg_active.p);
                        return dm_grad_eval(h, P, A, (const int32_t*)h->dmg_active.p);
                      },
                      [&](uint64_t it) {
                        hipLaunchKernelGGL(it == 1 ? k_sl_step<true> : k_sl_step<false>, dim3((unsigned)B), dim3(64), 0, h->stream, T, O);
                      });
}

// run_lbfgs in the exact channel mode, in the shape of stream_run_lbfgs: an env-step optimises the pre-action circuits
// under a plan of their own (dmb_pre), then the float32 round trip and one energy evaluation of the full circuits.
int dm_run_lbfgs(vqe_t* h, bool env_step, const vqe_lbfgs_opts_t& o) {
  VQE_TRY(dm_refusal(h));
  VQE_TRY(dm_prepare_ham(h));
  BatchArgs A = make_args(h);
  A.maxfun = o.maxfun;
  std::vector<int32_t> nfev;
  int64_t before[4], grad_info[4] = {0, 0, 0, 0};
  std::copy(h->dm_info, h->dm_info + 4, before);
  bool started = false;
  const int rc = minimize_or_env_step(h, env_step, A, nfev,
      [&](BatchArgs& a, const PreActionBatch* pre, std::vector<double>& x, std::vector<double>& f, std::vector<int32_t>& nf) {
        DmPlanSlot& P = pre ? h->dmb_pre : h->dmb_full;
        VQE_TRY(pre ? dm_batch_plan(h, P, pre->gates, pre->gbeg, pre->gcnt)
                    : dm_batch_plan(h, P, h->h_gates, h->h_gate_begin, h->h_gate_count));
        VQE_TRY(dm_grad_reserve(h, P));
        std::copy(h->dm_info, h->dm_info + 4, grad_info);
        started = true;
        h->last_run_dm = false;
        h->lb_batch = 0;
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        return dm_lbfgs(h, P, a, o, x, f, nf);
      },
      [&](const BatchArgs& a) {
        VQE_TRY(dm_batch_plan(h, h->dmb_full, h->h_gates, h->h_gate_begin, h->h_gate_count));
        VQE_TRY(dm_batch_reserve(h));
        return dm_batch_eval(h, h->dmb_full, a, nullptr);
      });
  if (rc) {
    if (!started) std::copy(before, before + 4, h->dm_info);
    return rc;
  }
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  std::copy(grad_info, grad_info + 4, h->dm_info);      // the resident count and the chunks of the gradient evaluations
  h->dm_info[2] = *std::max_element(nfev.begin(), nfev.end()) + (env_step ? 1 : 0);
  h->dm_info[3] = h->dmb_full.max_blocks;
  h->dm_blocks_last = h->dmb_full.max_blocks;
  h->lb_batch = h->batch;
  return VQE_OK;
}

// A Kraus override (vqe_set_noise_kraus) has no trajectory form: with one installed only the exact channel mode runs,
// and no state vector is handed out in any mode.  Checked before anything is loaded or launched.
// traj_ok: the call is one that quantum-jump trajectories serve (vqe_set_kraus_traj, vqe_qjump.h) - energies, COBYLA runs
// and env-steps in mode 0, states in either mode; then only what that path cannot hold is refused.
int kraus_refusal(vqe_t* h, bool state_call, bool traj_ok = false) {
  if (!h->kraus.any()) return VQE_OK;
  if (traj_ok && h->kraus_traj >= 1 && (state_call || h->noise_mode != 1)) {
    if (h->shard_world > 1 || h->amp_world > 1)
      return fail(h, VQE_ESTATE, "quantum-jump trajectories of a Kraus channel (vqe_set_kraus_traj) take no term- or amplitude-sharded handle");
    if (!h->lds_path && h->sq_resident == 0)
      return fail(h, VQE_ESTATE, "quantum-jump trajectories of a Kraus channel (vqe_set_kraus_traj) run for n_qubits <= 13 (LDS-resident path) only");
    return VQE_OK;
  }
  if (state_call) return fail(h, VQE_ESTATE, "a Kraus channel (vqe_set_noise_kraus) has no state vector: vqe_get_state* is refused while it is installed");
  if (h->noise_mode != 1)
    return fail(h, VQE_ESTATE, "a Kraus channel (vqe_set_noise_kraus) has no Pauli-trajectory form: use the exact channel mode (vqe_set_noise_mode 1)");
  return VQE_OK;
}

// The evaluation trace of an optimiser run (vqe_batch_set_trace): [batch][maxfun][1 + max_params] doubles, zeroed
int arm_trace(vqe_t* h, BatchArgs& A, int maxfun) {
  const size_t stride = (size_t)1 + (size_t)h->max_params, words = (size_t)h->batch * (size_t)maxfun * stride;
  HIP_TRY(h, h->d_trace.reserve(words));
  HIP_TRY(h, hipMemsetAsync(h->d_trace.p, 0, words * sizeof(double), h->stream));
  A.trace = h->d_trace.p;
  h->trace_maxfun = maxfun; h->trace_stride = (int)stride; h->trace_batch = h->batch;
  return VQE_OK;
}

// ---- quantum-jump trajectories of a Kraus override in mode 0 (vqe_set_kraus_traj; kernels: vqe_qjump.h) ----

int build_grad_tables(vqe_t* h);      // (below: the GradHam tables of the adjoint kernels, whose energy step this path runs)

// The run is served by trajectories: the switch, an override, and mode 0 (a state: either mode)
bool qj_serves(const vqe_t* h, Run mode) {
  return h->kraus_traj >= 1 && h->kraus.any() && mode != Run::Reduce && (mode == Run::State || h->noise_mode != 1);
}

// The channel tables of the two slots: the override, else the Pauli set of a table (vqe_set_noise_pauli), else the
// depolarising Kraus set of p1 / p2 (none at probability 0)
int qj_prepare(vqe_t* h) {
  if (h->qj_tab_ver == h->qj_ver) return VQE_OK;
  std::vector<cplx> dep;
  std::vector<double> k1, w1, k2, w2;
  h->qj_n1 = h->channels.n1;
  h->qj_n2 = h->channels.n2;
  if (h->channels.n1 > 0) {
    qj_build_tables(h->channels.K1.data(), h->channels.n1, 2, k1, w1);
  } else if (h->noise.p1 > 0.0) {
    qj_depol_kraus(h->noise.p1, 2, dep);
    qj_build_tables(dep.data(), h->qj_n1 = 4, 2, k1, w1);
  }
  if (h->channels.n2 > 0) {
    qj_build_tables(h->channels.K2.data(), h->channels.n2, 4, k2, w2);
  } else if (h->noise.p2 > 0.0) {
    qj_depol_kraus(h->noise.p2, 4, dep);
    qj_build_tables(dep.data(), h->qj_n2 = 16, 4, k2, w2);
  }
  VQE_TRY(upload(h, h->qj_K1, k1));
  VQE_TRY(upload(h, h->qj_W1, w1));
  VQE_TRY(upload(h, h->qj_K2, k2));
  VQE_TRY(upload(h, h->qj_W2, w2));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // host vectors go out of scope
  h->qj_tab_ver = h->qj_ver;
  return VQE_OK;
}

// One evaluation: T trajectories of every active circuit of the batch A describes at A.theta with evaluation id eval_id,
// their mean into A.fout.  Queued on the handle's stream; nothing is copied back.  state_out: the state of work item 0.
int qj_eval(vqe_t* h, const BatchArgs& A, int T, uint64_t eval_id, const int32_t* active, int32_t* nfev, double2* state_out) {
  const int B = A.batch;
  HIP_TRY(h, h->qj_e.reserve((size_t)B * T));
  HIP_TRY(h, h->qj_jumps.reserve((size_t)B * T));
  HIP_TRY(h, h->qj_jsum.reserve(B));
  const QjDev Q{h->qj_n1, h->qj_n2, h->qj_K1.p, h->qj_W1.p, h->qj_K2.p, h->qj_W2.p, T, eval_id, active,
                h->qj_e.p, h->qj_jumps.p, state_out};
  int grid = 0, wg_per_cu = 1;
  hipError_t herr = hipSuccess;
  const int rc = qj_launch(A, h->gham, Q, nfev, h->qj_jsum.p, h->lds_per_cu, h->cu_count, h->stream, &grid, &wg_per_cu, &herr);
  if (rc == QJ_ETOOLARGE) return fail(h, VQE_EINVAL, "circuit too large for the trajectory kernel (gates + parameters)");
  if (rc == QJ_ESIZE) return fail(h, VQE_EINVAL, "quantum-jump trajectories run for n_qubits <= 13 (LDS-resident path) only");
  HIP_TRY(h, herr);
  h->last_wg_per_cu = std::min(8, wg_per_cu);
  h->qj_info[1] = grid;
  h->qj_jsum_batch = B;
  return VQE_OK;
}

// qj_eval on the streaming path (n >= 14, vqe_set_stream_kraus_traj; kernels: vqe_stream_qjump.h): the B T work items
// are virtual streams with their states in HBM, resident a chunk at a time.  Per chunk: the lock-step rounds `size`
// counts (sq_trajectories), the frame of every stream in the layout of the streaming path, and that path's own
// Pauli-term reduction on the virtual batch, whose energies are the chunk's slice of qj_e.  The mean after the last
// chunk.  Every circuit is evaluated, waited for or not: `active` only keeps f and the jump sums of the others.
int sq_eval(vqe_t* h, const BatchArgs& A, const SqSize& size, int T, uint64_t eval_id, const int32_t* active, int32_t* nfev,
            double2* state_out) {
  const int B = A.batch, n = h->n;
  const size_t dim = (size_t)1 << n, total = (size_t)B * T;
  const size_t blocks = (size_t)sq_blocks(n);
  if (h->sq_resident < 0 && !h->sq_auto_cap) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    h->sq_auto_cap = std::max<size_t>(1, (free_b / 4) / (dim * sizeof(double2) + (blocks * 16 + 32) * sizeof(double)));
  }
  const size_t cap = h->sq_resident > 0 ? (size_t)h->sq_resident : h->sq_auto_cap;
  const int R = (int)std::min<size_t>(std::min<size_t>(cap, total), 65535);      // a chunk is the y extent of a grid
  StreamWork& sw = h->sw;
  HIP_TRY(h, sw.states.reserve((size_t)R * dim));
  HIP_TRY(h, sw.masks.reserve((size_t)R * 64));
  HIP_TRY(h, sw.meta.reserve((size_t)R * 8));
  HIP_TRY(h, h->sq_ops.reserve((size_t)B * A.max_ops));
  HIP_TRY(h, h->sq_jpos.reserve((size_t)B * A.max_ops));
  HIP_TRY(h, h->sq_masks.reserve((size_t)B * 64));
  HIP_TRY(h, h->sq_meta.reserve((size_t)B * 8));
  HIP_TRY(h, h->sq_cs.reserve((size_t)B * A.max_params));
  HIP_TRY(h, h->sq_part.reserve((size_t)R * blocks * 16));
  HIP_TRY(h, h->sq_kmat.reserve((size_t)R * 32));
  HIP_TRY(h, h->qj_e.reserve(total));
  HIP_TRY(h, h->qj_jumps.reserve(total));
  HIP_TRY(h, h->qj_jsum.reserve(B));
  HIP_TRY(h, sq_compile(A, h->qj_n1 > 0, h->qj_n2 > 0, h->sq_ops.p, h->sq_masks.p, h->sq_meta.p, h->sq_jpos.p, h->sq_cs.p, h->stream));
  HIP_TRY(h, hipMemsetAsync(h->qj_jumps.p, 0, total * sizeof(int32_t), h->stream));
  SqDev D{};
  D.n = n; D.T = T;
  D.states = sw.states.p; D.init = A.init;
  D.ops = h->sq_ops.p; D.meta = h->sq_meta.p; D.jpos = h->sq_jpos.p; D.cs = h->sq_cs.p;
  D.max_ops = A.max_ops; D.max_params = A.max_params;
  D.part = h->sq_part.p; D.kmat = h->sq_kmat.p; D.jumps = h->qj_jumps.p;
  D.n1 = h->qj_n1; D.n2 = h->qj_n2;
  D.K1 = h->qj_K1.p; D.W1 = h->qj_W1.p; D.K2 = h->qj_K2.p; D.W2 = h->qj_W2.p;
  D.seed = A.noise.seed; D.eval_id = eval_id;
  // the virtual batch of the energy: no circuit of its own (the plans are made per chunk), no noise, no shot term
  BatchArgs V = A;
  V.noise.p1 = V.noise.p2 = 0.0;
  V.noise.pauli = nullptr;
  V.noise.shot_sigma = 0.0;
  int grid = 0;
  for (size_t c0 = 0; c0 < total; c0 += (size_t)R) {
    D.cnt = (int)std::min<size_t>((size_t)R, total - c0);
    D.w0 = (long long)c0;
    HIP_TRY(h, sq_trajectories(D, size, h->stream, &grid));
    HIP_TRY(h, sq_frames(D, h->sq_masks.p, sw.masks.p, sw.meta.p, h->stream));
    V.batch = D.cnt;
    V.fout = h->qj_e.p + c0;
    sw.plan_ops_ok = sw.plan_energy_ok = false;
    VQE_TRY(evaluate(h, V, eval_id, StreamWant::Energy));
    if (state_out && c0 == 0) {
      hipLaunchKernelGGL(k_s_state_out, dim3((unsigned)(dim / kThreads)), dim3(kThreads), 0, h->stream, A, sw.states.p, sw.masks.p,
                         sw.meta.p);
      HIP_TRY(h, hipGetLastError());
    }
  }
  sw.plan_ops_ok = sw.plan_energy_ok = false;      // (the plans of the last chunk are no circuit's of the resident batch)
  HIP_TRY(h, sq_mean(B, T, h->qj_e.p, h->qj_jumps.p, active, A.noise, eval_id, A.fout, nfev, h->qj_jsum.p, h->stream));
  h->qj_info[1] = grid;
  h->qj_jsum_batch = B;
  h->sq_info[0] = R;
  h->sq_info[1] = (int64_t)((total + (size_t)R - 1) / (size_t)R);
  h->sq_info[2] = size.rounds;
  h->sq_info[3] = (int64_t)sq_state_sweeps(size);
  return VQE_OK;
}

// Run::Energy / State / Minimize / EnvStep on trajectories, in the shape of dm_run_batched: the optimiser of every circuit
// lives on the device (k_s_cobyla through lockstep_cobyla), an evaluation is qj_eval.  The k-th evaluation of an
// optimiser run draws at counter + k, the final full-circuit evaluation of an env-step at counter + maxfun + 1.
int qj_run(vqe_t* h, Run mode, BatchArgs A) {
  const bool streaming = !h->lds_path;      // (n >= 14: vqe_set_stream_kraus_traj, sq_eval)
  if (!streaming) VQE_TRY(build_grad_tables(h));
  VQE_TRY(qj_prepare(h));
  const int T = h->kraus_traj;
  const uint64_t base = h->noise.eval_base;
  // the streaming path's loop is sized on the host, by the walk of the batch an evaluation runs
  const auto size_of = [&](const std::vector<GateRec>& g, const std::vector<int64_t>& gbeg, const std::vector<int32_t>& gcnt, int batch) {
    return streaming ? sq_size(g.data(), gbeg.data(), gcnt.data(), batch, h->n, h->qj_n1 > 0, h->qj_n2 > 0) : SqSize{};
  };
  const SqSize full = size_of(h->h_gates, h->h_gate_begin, h->h_gate_count, mode == Run::State ? 1 : h->batch);
  const auto eval = [h, streaming](const BatchArgs& a, const SqSize& size, int n_traj, uint64_t id, const int32_t* active, int32_t* nf,
                                   double2* state_out) {
    return streaming ? sq_eval(h, a, size, n_traj, id, active, nf, state_out) : qj_eval(h, a, n_traj, id, active, nf, state_out);
  };
  h->qj_traj_batch = 0;
  h->qj_info[0] = T;
  h->qj_info[3] = 1;
  if (streaming) h->stream_states_undone = true;      // (the states this run leaves are no batch's a reduction-only launch may take)
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  if (mode == Run::Energy) {
    VQE_TRY(eval(A, full, T, base, nullptr, A.nfev, nullptr));
    h->qj_traj_batch = h->batch;
  } else if (mode == Run::State) {
    A.batch = 1;                                  // trajectory 0 of the one circuit
    VQE_TRY(eval(A, full, 1, base, nullptr, nullptr, A.state_out));
  } else {
    std::vector<int32_t> nfev;
    VQE_TRY(minimize_or_env_step(h, mode == Run::EnvStep, A, nfev,
        [&](BatchArgs& a, const PreActionBatch* pre, std::vector<double>& x, std::vector<double>& f, std::vector<int32_t>& nf) {
          const SqSize size = pre ? size_of(pre->gates, pre->gbeg, pre->gcnt, h->batch) : full;
          return lockstep_cobyla(h, a, x, f, nf, [&eval, size, T, base](const BatchArgs& t, uint64_t it, const int32_t* active) {
            return eval(t, size, T, base + it, active, nullptr, nullptr);
          });
        },
        [&](const BatchArgs& a) { return eval(a, full, T, base + (uint64_t)a.maxfun + 1, nullptr, nullptr, nullptr); }));
    h->qj_info[3] = *std::max_element(nfev.begin(), nfev.end()) + (mode == Run::EnvStep ? 1 : 0);
    if (mode == Run::EnvStep) h->qj_traj_batch = h->batch;
  }
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  return VQE_OK;
}

int run(vqe_t* h, Run mode, double rhobeg, double rhoend, int maxfun) {
  VQE_TRY(kraus_refusal(h, mode == Run::State, mode != Run::Reduce));
  HIP_TRY(h, hipSetDevice(h->dev));
  BatchArgs A = make_args(h);
  A.rhobeg = rhobeg; A.rhoend = rhoend; A.maxfun = maxfun;
  const bool optimise = mode == Run::Minimize || mode == Run::EnvStep;
  if (optimise && (h->shard_world > 1 || h->amp_world > 1))
    return fail(h, VQE_ESTATE, "term-sharded handles hold partial energies: drive COBYLA with "
                               "vqe_cobyla_ask/tell and sum the partial energies of all ranks");
  if (mode == Run::Reduce && h->lds_path)
    return fail(h, VQE_ESTATE, "the reduction-only launch exists on the streaming path (n >= 14) only");
  // Everything else a run can be refused for, before the trace, the L-BFGS info and the timing of the previous run are
  // given up: a refused run leaves the handle and what can be fetched from it as they were.
  const bool exact = h->noise_mode == 1 && (mode == Run::Energy || optimise);
  const bool traj = qj_serves(h, mode);
  if (traj) {
    if (h->lds_path && qj_lds_bytes(h->n, A.max_ops, A.max_params) > (size_t)h->lds_per_cu)
      return fail(h, VQE_EINVAL, "circuit too large for the trajectory kernel (gates + parameters)");
  } else if (exact) {
    VQE_TRY(dm_refusal(h));
  } else if (h->lds_path) {
    const size_t lds = lds_bytes(h->n, A.max_ops, A.max_params, A.ham.n_groups, A.max_pair, optimise && wide_launch(h->n, A.max_params));
    if (const char* why = lds_launch_refusal(h->n, lds, A.max_ops, (size_t)h->lds_per_cu)) return fail(h, VQE_EINVAL, why);
  } else if (mode == Run::Reduce) {
    if (h->stream_states_undone)
      return fail(h, VQE_ESTATE, "the states of the last run were undone by its gradient sweep: run the energy first");
    if (h->sw.states.cap < ((size_t)h->batch << h->n)) return fail(h, VQE_ESTATE, "no states: run the energy first");
  }
  if (h->trace_on && optimise && h->lds_path && !traj) VQE_TRY(arm_trace(h, A, maxfun));
  h->last_run_dm = false;
  h->lb_batch = 0;             // fout / nfev are about to be another run's: the L-BFGS info of an earlier one is stale
  h->qj_traj_batch = 0;        // ... and so are the per-trajectory energies of an earlier trajectory run
  if (exact && !traj) return dm_run(h, mode, A);
  VQE_TRY(traj ? qj_run(h, mode, A) : h->lds_path ? dispatch_lds(h, mode, A) : stream_run(h, mode, A));
  // every evaluation of a stochastic run consumes fresh trajectory numbers
  if (mode != Run::Reduce) h->noise.eval_base += (optimise ? (uint64_t)maxfun + 1 : 1);
  return VQE_OK;
}

// ---- adjoint gradient (vqe_grad.h) -----------------------------------------------------------
// The unit-free table set of k_lds_energy_grad (plan_grad_tables, ham_layout.h), rebuilt when the Hamiltonian or its
// shard changed.
int build_grad_tables(vqe_t* h) {
  if (h->grad_ham_ver == h->ham_ver) return VQE_OK;
  GradTables T;
  plan_grad_tables(h->ham_host, h->n, h->lds_path, h->shard_rank, h->shard_world, T);
  VQE_TRY(upload(h, h->g_gx, T.gx));
  VQE_TRY(upload(h, h->g_off, T.off));
  VQE_TRY(upload(h, h->g_cplx, T.cplx));
  VQE_TRY(upload(h, h->g_tab, T.tab));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // host vectors go out of scope
  h->gham = GradHam{(int)T.gx.size(), h->g_gx.p, h->g_off.p, h->g_cplx.p, h->g_tab.p};
  h->grad_ham_ver = h->ham_ver;
  return VQE_OK;
}

// What the adjoint kernels cannot serve: a gradient of a stochastic trajectory is of no use to an optimiser, and the
// streaming path (n >= 14) computes gradients only after vqe_set_stream_grad (a second state-sized buffer per stream).
// Checked before anything is loaded, so a refused call leaves the handle as it was.
// noise_grad_on: the run is the mean over frozen Pauli-noise realisations (after grad_state_refusal let it through).
// (grad_state_refusal: everything but the path test - the device L-BFGS has a switch of its own for n >= 14)
constexpr int kStreamNoiseGradMaxQubits = 20;      // the sizes the streaming form of the noisy gradient is served at
NoiseGradVerdict noise_grad_state(const vqe_t* h) {
  return noise_grad_verdict(NoiseGradState{h->noise_grad_T, h->noise_mode, pauli_noise_on(h), h->lds_path,
                                           !h->lds_path && h->n <= kStreamNoiseGradMaxQubits && h->sng_resident != 0});
}
bool noise_grad_on(const vqe_t* h) { return noise_grad_state(h) == NG_SERVED; }
bool noise_grad_stream(const vqe_t* h) { return noise_grad_state(h) == NG_SERVED_STREAM; }      // (n >= 14: vqe_set_stream_noise_grad)
NoiseGrad noise_grad_args(const vqe_t* h) {
  return noise_grad_on(h) ? NoiseGrad{h->noise_grad_T, std::max(1, h->max_rot)} : NoiseGrad{0, -1};
}
int grad_state_refusal(vqe_t* h) {
  if (h->noise_mode == 1 && h->dm_grad) {
    // the exact channel mode after vqe_set_dm_grad: deterministic energies whatever p1 / p2, no shot noise in this mode;
    // the gates and the size are dm_refusal's, checked once the batch is known
    if (h->dm_batched == 0)
      return fail(h, VQE_ESTATE, "energy gradients in the exact channel noise mode are computed on the batched path: "
                                 "vqe_set_dm_grad needs vqe_set_dm_batched != 0 beside it");
    if (h->amp_world > 1) return fail(h, VQE_ESTATE, "the exact channel mode has no amplitude sharding");
    return VQE_OK;
  }
  VQE_TRY(kraus_refusal(h, false));
  // frozen realisations (vqe_set_noise_grad, noise_grad_host.h): served in mode 0 on the LDS-resident path; shot noise
  // and shards are refused below as without noise
  const NoiseGradVerdict ng = noise_grad_state(h);
  if (ng == NG_REFUSED_OFF)
    return fail(h, VQE_ESTATE, "energy gradients of Pauli-noise trajectories are refused (set p1 = p2 = 0, or in noise mode 0 "
                               "freeze the draws: vqe_set_noise_grad)");
  if (ng == NG_REFUSED_PATH)
    return fail(h, VQE_ESTATE, "energy gradients of Pauli-noise trajectories (vqe_set_noise_grad) are computed for "
                               "n_qubits <= 13 (LDS-resident path) only");
  if (h->noise_mode == 1) return fail(h, VQE_ESTATE, "energy gradients are not available in the exact channel noise mode");
  if (h->noise.shot_sigma != 0.0) return fail(h, VQE_ESTATE, "energy gradients with shot noise are refused (set sigma_total = 0)");
  if (h->amp_world > 1) return fail(h, VQE_ESTATE, "energy gradients of an amplitude shard are refused");
  return VQE_OK;
}
int grad_refusal(vqe_t* h) {
  if (h->noise_mode == 1 && h->dm_grad) return grad_state_refusal(h);
  if (!h->lds_path && h->sq_resident != 0) VQE_TRY(kraus_refusal(h, false));      // (trajectories on: the override refuses, as at n <= 13)
  if (!h->lds_path && !h->stream_grad)
    return fail(h, VQE_EINVAL, "energy gradients are computed for n_qubits <= 13 (LDS-resident path) only");
  return grad_state_refusal(h);
}

// The launch of the two adjoint kernels (the gradient, the device L-BFGS): both come as <N, LAM_GLOBAL> pairs that take
// (A, gham, x, lambda scratch) and size their LDS by a formula of grad_lds_bytes' form.  lambda lives in the LDS unless
// N >= 13 or psi + lambda + ops exceed it; in global memory it is one slice per workgroup of a persistent grid.
// prepare(grid, x): what the caller has to size by the chosen grid (a hipError_t).
// ng: {T, rows of gacc} of the NOISY instances (the caller passes those kernels), {0, -1} for the noiseless ones.
template <int N, class X, class Prepare>
int launch_adjoint(vqe_t* h, const BatchArgs& A, NoiseGrad ng, size_t (*lds_bytes)(int, bool, int, int, int, int),
                   void (*k_global)(BatchArgs, GradHam, X, double2*, NoiseGrad), void (*k_lds)(BatchArgs, GradHam, X, double2*, NoiseGrad),
                   const char* too_large, X x, Prepare prepare) {
  constexpr int NW = Geo<N>::NW;
  bool lam_global = N >= 13;
  size_t lds = lds_bytes(N, lam_global, A.max_ops, A.max_params, NW, ng.rows);
  if (!lam_global && lds > (size_t)h->lds_per_cu) {      // psi + lambda + ops do not fit: lambda moves to global memory
    lam_global = true;
    lds = lds_bytes(N, true, A.max_ops, A.max_params, NW, ng.rows);
  }
  if (lds > (size_t)h->lds_per_cu) return fail(h, VQE_EINVAL, too_large);
  const int wg_per_cu = std::max(1, (int)(h->lds_per_cu / lds));
  const auto kernel = lam_global ? k_global : k_lds;
  HIP_TRY(h, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  h->last_wg_per_cu = std::min(8, wg_per_cu);
  int grid = A.batch;
  if (lam_global) {
    grid = std::min(A.batch, h->cu_count * wg_per_cu);
    HIP_TRY(h, h->g_lam.reserve((size_t)grid << N));
  }
  HIP_TRY(h, prepare(grid, x));
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(Geo<N>::NT), lds, h->stream, A, h->gham, x, lam_global ? h->g_lam.p : (double2*)nullptr, ng);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  return VQE_OK;
}

template <int N>
int launch_grad(vqe_t* h, const BatchArgs& A) {
  const NoiseGrad ng = noise_grad_args(h);
  const char* too_large = "circuit too large for the adjoint gradient kernel (gates + parameters)";
  const auto prepare = [](int, double*) { return hipSuccess; };
  if (ng.rows >= 0)
    return launch_adjoint<N>(h, A, ng, grad_lds_bytes, k_lds_energy_grad<N, true, true>, k_lds_energy_grad<N, false, true>,
                             too_large, h->d_grad.p, prepare);
  return launch_adjoint<N>(h, A, ng, grad_lds_bytes, k_lds_energy_grad<N, true, false>, k_lds_energy_grad<N, false, false>,
                           too_large, h->d_grad.p, prepare);
}

// The resident (circuit, realisation) pairs a noisy streaming gradient may hold: max_resident as set, or with -1 what a
// quarter of the free device memory takes (psi, lambda and the backward sweep's partials per pair), fixed at the first run.
int stream_noise_cap(vqe_t* h, const BatchArgs& A, int64_t* cap) {
  if (h->sng_resident < 0 && !h->sng_auto_cap) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    const size_t dim = (size_t)1 << h->n;
    const size_t gblk = ((dim >> kGradOpsPerSweep) + kThreads - 1) / kThreads;
    const size_t per_pair = 2 * dim * sizeof(double2) + (size_t)A.max_ops * gblk * sizeof(double);
    h->sng_auto_cap = std::max<size_t>(1, (free_b / 4) / per_pair);
  }
  *cap = h->sng_resident > 0 ? (int64_t)h->sng_resident : (int64_t)h->sng_auto_cap;
  return VQE_OK;
}

// One evaluation of E_T and its gradient on the streaming path (vqe_stream_grad.h: stream_noise_energy_grad): the
// realisations eval_base .. eval_base + T - 1 of the batch A describes at A.theta, E_T into A.fout, the gradient into d_grad.
int stream_noise_grad_eval(vqe_t* h, const BatchArgs& A) {
  int64_t cap = 1;
  VQE_TRY(stream_noise_cap(h, A, &cap));
  int used = 0, chunks = 0;
  VQE_TRY(stream_noise_energy_grad(h->sw, h->snw, A, h->stream, h->noise.eval_base, h->noise_grad_T, cap, h->d_grad.p, h->err,
                                   h->gen, &used, &chunks));
  h->sng_info[0] = h->sng_resident;
  h->sng_info[1] = used;
  h->sng_info[2] = chunks;
  h->sng_info[3] = 0;
  return VQE_OK;
}

// Streaming path (n >= 14, vqe_set_stream_grad): forward sweeps, lambda = H psi, backward sweeps (vqe_stream_grad.h);
// under Pauli noise (vqe_set_stream_noise_grad) the mean over the frozen realisations, the counter as at n <= 13
int stream_grad(vqe_t* h, const BatchArgs& A) {
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  h->stream_states_undone = true;
  if (noise_grad_stream(h)) {
    VQE_TRY(stream_noise_grad_eval(h, A));
    h->noise.eval_base += noise_grad_consumed(NoiseGradRun::Gradient, h->noise_grad_T, h->noise_grad_hold);
  } else {
    VQE_TRY(stream_energy_grad(h->sw, A, h->stream, h->noise.eval_base, h->d_grad.p, h->err, h->gen));
  }
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  return VQE_OK;
}

int run_grad(vqe_t* h) {
  VQE_TRY(grad_refusal(h));
  if (dm_grad_path(h)) return dm_run_grad(h);
  HIP_TRY(h, hipSetDevice(h->dev));
  if (h->lds_path) VQE_TRY(build_grad_tables(h));
  HIP_TRY(h, h->d_grad.reserve((size_t)h->total_params + 1));
  const BatchArgs A = make_args(h);
  h->last_run_dm = false;
  h->qj_traj_batch = 0;
  if (!h->lds_path) return stream_grad(h, A);
  VQE_TRY(dispatch_n(h, "energy gradients are computed for n_qubits <= 13 (LDS-resident path) only",
                     [&](auto n) -> int { return launch_grad<decltype(n)::value>(h, A); }, LdsSizes{}));
  // frozen realisations: the launch read ids eval_base .. eval_base + T - 1 (a held counter waits for vqe_noise_grad_advance)
  if (noise_grad_on(h)) h->noise.eval_base += noise_grad_consumed(NoiseGradRun::Gradient, h->noise_grad_T, h->noise_grad_hold);
  return VQE_OK;
}

// ---- device L-BFGS (vqe_lbfgs.h) -------------------------------------------------------------
// Everything a run of k_lds_minimize_lbfgs can be refused for, checked before anything is loaded or launched; *o
// receives the options (NULL: the defaults).
int lbfgs_check(vqe_t* h, const vqe_lbfgs_opts_t* opts, vqe_lbfgs_opts_t* o) {
  (void)vqe_lbfgs_default_opts(o);
  if (opts) *o = *opts;
  if (h->amp_world > 1) return fail(h, VQE_ESTATE, "the device L-BFGS takes no amplitude shard");      // (only n >= 14 can hold one)
  if (!h->lds_path && h->sq_resident != 0) VQE_TRY(kraus_refusal(h, false));      // (as in grad_refusal)
  if (!h->lds_path && !h->stream_lbfgs)      // (with or without vqe_set_stream_grad: the optimiser has a switch of its own)
    return fail(h, VQE_EINVAL, "the device L-BFGS runs for n_qubits <= 13 (LDS-resident path) only; "
                               "n_qubits >= 14 after vqe_set_stream_lbfgs");
  VQE_TRY(grad_state_refusal(h));
  if (h->shard_world > 1)
    return fail(h, VQE_ESTATE, "term-sharded handles hold partial energies: the line search of the device L-BFGS needs the full energy");
  if (o->history < 1 || o->history > kLbfgsMaxHistory) return fail(h, VQE_EINVAL, "L-BFGS history must be in [1, 16]");
  if (o->maxiter < 0 || o->maxfun < 1 || o->max_ls < 1) return fail(h, VQE_EINVAL, "L-BFGS needs maxiter >= 0, maxfun >= 1, max_ls >= 1");
  if (!(o->gtol >= 0.0) || !(o->ftol >= 0.0)) return fail(h, VQE_EINVAL, "L-BFGS tolerances must be >= 0");
  if (!(o->c1 > 0.0 && o->c1 < 1.0)) return fail(h, VQE_EINVAL, "L-BFGS c1 must be in (0, 1)");
  return VQE_OK;
}

template <int N>
int launch_lbfgs(vqe_t* h, const BatchArgs& A, const LbfgsArgs& O) {
  const NoiseGrad ng = noise_grad_args(h);
  const char* too_large = "circuit too large for the device L-BFGS kernel (gates + parameters)";
  const auto prepare = [&](int grid, LbfgsArgs& o) {      // the optimiser's vectors: one slice per workgroup
    const hipError_t e = h->lb_work.reserve((size_t)grid * lbfgs_work_doubles(A.max_params, o.m));
    o.work = h->lb_work.p;
    return e;
  };
  if (ng.rows >= 0)
    return launch_adjoint<N>(h, A, ng, lbfgs_lds_bytes, k_lds_minimize_lbfgs<N, true, true>, k_lds_minimize_lbfgs<N, false, true>,
                             too_large, O, prepare);
  return launch_adjoint<N>(h, A, ng, lbfgs_lds_bytes, k_lds_minimize_lbfgs<N, true, false>, k_lds_minimize_lbfgs<N, false, false>,
                           too_large, O, prepare);
}

// The device L-BFGS of all resident streams in lock-step (vqe_stream_lbfgs.h) through lockstep_run: an evaluation is
// stream_energy_grad on the trial points (E into d_f, the gradient into d_grad), the step kernel k_sl_step, whose FIRST
// form takes the evaluation of x0.  A: the batch to optimise (its par_begin / par_count lay out x); x: in x0, out the
// result; nit / status stay on the device (lb_nit / lb_status).  The last launch is a gradient: the states are the
// undone ones.
int stream_lbfgs(vqe_t* h, BatchArgs& A, const vqe_lbfgs_opts_t& o, std::vector<double>& x, std::vector<double>& f,
                 std::vector<int32_t>& nfev) {
  const int B = h->batch;
  HIP_TRY(h, h->d_grad.reserve(x.size() + 1));
  HIP_TRY(h, h->lb_work.reserve((size_t)B * lbfgs_work_doubles(A.max_params, o.history)));
  HIP_TRY(h, h->lb_nit.reserve(B));
  HIP_TRY(h, h->lb_status.reserve(B));
  HIP_TRY(h, h->lb_rec.reserve(B));
  VQE_TRY(lockstep_begin(h, A, x));
  const StreamLbfgsArgs T{A.par_begin, A.par_count, A.max_params, h->lb_rec.p, h->d_x.p, h->d_f.p, h->d_grad.p,
                          h->ls_running.p, h->ls_xres.p, h->ls_fres.p, h->ls_nfres.p};
  const LbfgsArgs O{o.history, o.maxiter, o.maxfun, o.max_ls, o.gtol, o.ftol, o.c1, h->lb_work.p, h->lb_nit.p, h->lb_status.p};
  h->stream_states_undone = true;
  return lockstep_run(h, "L-BFGS", o.maxfun, x, f, nfev,
                      [&](uint64_t it) {      // (frozen realisations: the same T ids at every trial point)
                        if (noise_grad_stream(h)) return stream_noise_grad_eval(h, A);
                        return stream_energy_grad(h->sw, A, h->stream, h->noise.eval_base + it, h->d_grad.p, h->err, h->gen);
                      },
                      [&](uint64_t it) {
                        hipLaunchKernelGGL(it == 1 ? k_sl_step<true> : k_sl_step<false>, dim3((unsigned)B), dim3(64), 0, h->stream, T, O);
                      });
}

// run_lbfgs on the streaming path (n >= 14, vqe_set_stream_lbfgs).  env_step: the rule of the streaming Run::EnvStep with
// the L-BFGS in COBYLA's place - pre-action circuits built on the host (the kernel knows no hole), float32 round trip,
// one evaluation of the full circuits.
int stream_run_lbfgs(vqe_t* h, bool env_step, const vqe_lbfgs_opts_t& o) {
  BatchArgs A = make_args(h);
  A.maxfun = o.maxfun;
  h->last_run_dm = false;
  h->lb_batch = 0;
  std::vector<int32_t> nfev;
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  // (frozen realisations: the closing energy of an env-step is the single trajectory with id eval_base + T)
  const bool frozen = noise_grad_stream(h);
  const uint64_t eval_id = h->noise.eval_base + (frozen ? (uint64_t)h->noise_grad_T : (uint64_t)o.maxfun + 1);
  VQE_TRY(minimize_or_env_step(h, env_step, A, nfev,
      [&](BatchArgs& a, const PreActionBatch*, std::vector<double>& x, std::vector<double>& f, std::vector<int32_t>& nf) {
        return stream_lbfgs(h, a, o, x, f, nf);
      },
      [h, eval_id](const BatchArgs& a) { return evaluate(h, a, eval_id, StreamWant::Both); }));
  if (env_step) h->stream_states_undone = false;      // (the last launch was an energy: the states are those of the full circuits)
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  h->lb_batch = h->batch;
  if (frozen)
    h->noise.eval_base += noise_grad_consumed(env_step ? NoiseGradRun::EnvStepLbfgs : NoiseGradRun::Lbfgs, h->noise_grad_T, h->noise_grad_hold);
  return VQE_OK;
}

// o: options that passed lbfgs_check
int run_lbfgs(vqe_t* h, bool env_step, const vqe_lbfgs_opts_t& o) {
  HIP_TRY(h, hipSetDevice(h->dev));
  if (dm_grad_path(h)) return dm_run_lbfgs(h, env_step, o);
  if (!h->lds_path) return stream_run_lbfgs(h, env_step, o);
  VQE_TRY(build_grad_tables(h));
  BatchArgs A = make_args(h);
  A.maxfun = o.maxfun;
  if (env_step) set_env_step(h, A);
  if (h->trace_on) VQE_TRY(arm_trace(h, A, o.maxfun));
  HIP_TRY(h, h->lb_nit.reserve(h->batch));
  HIP_TRY(h, h->lb_status.reserve(h->batch));
  const LbfgsArgs O{o.history, o.maxiter, o.maxfun, o.max_ls, o.gtol, o.ftol, o.c1, nullptr, h->lb_nit.p, h->lb_status.p};
  h->last_run_dm = false;
  h->lb_batch = 0;
  VQE_TRY(dispatch_n(h, "the device L-BFGS serves n_qubits <= 13 (LDS-resident path) only",
                     [&](auto n) -> int { return launch_lbfgs<decltype(n)::value>(h, A, O); }, LdsSizes{}));
  h->lb_batch = h->batch;
  // frozen realisations: every evaluation read ids eval_base .. eval_base + T - 1, an env-step's closing energy id eval_base + T
  if (noise_grad_on(h))
    h->noise.eval_base += noise_grad_consumed(env_step ? NoiseGradRun::EnvStepLbfgs : NoiseGradRun::Lbfgs, h->noise_grad_T, h->noise_grad_hold);
  return VQE_OK;
}

// ---- device Adam-SPSA (vqe_spsa.h) -----------------------------------------------------------
// Everything a run of k_lds_minimize_spsa can be refused for, checked before anything is loaded or launched; *o
// receives the options.
int spsa_check(vqe_t* h, const vqe_spsa_opts_t* opts, SpsaOpts* o) {
  if (!opts) return fail(h, VQE_EINVAL, "Adam-SPSA options are NULL (start from vqe_spsa_default_opts)");
  *o = SpsaOpts{opts->maxiter, opts->a, opts->alpha, opts->stability, opts->c, opts->gamma, opts->beta_1, opts->beta_2,
                opts->lamda, opts->eps, opts->seed};
  if (const char* why = spsa_bad_option(*o)) return fail(h, VQE_EINVAL, why);
  if (h->amp_world > 1) return fail(h, VQE_ESTATE, "the device Adam-SPSA takes no amplitude shard");      // (only n >= 14 can hold one)
  if (!h->lds_path)
    return fail(h, VQE_EINVAL, "the device Adam-SPSA runs for n_qubits <= 13 (LDS-resident path) only");
  if (h->noise_mode == 1)
    return fail(h, VQE_ESTATE, "the device Adam-SPSA optimises mode 0 energies: refused in the exact channel noise mode (vqe_set_noise_mode 1)");
  if (h->kraus.any())
    return fail(h, VQE_ESTATE, "the device Adam-SPSA has no quantum-jump form: refused while a Kraus channel (vqe_set_noise_kraus, "
                               "vqe_set_kraus_traj) is installed");
  if (h->shard_world > 1)
    return fail(h, VQE_ESTATE, "term-sharded handles hold partial energies: the device Adam-SPSA needs the full energy");
  return VQE_OK;
}

template <int N>
int launch_spsa(vqe_t* h, const BatchArgs& A, const SpsaOpts& o) {
  const size_t lds = spsa_lds_bytes(N, A.max_ops, A.max_params, A.ham.n_groups, A.max_pair);
  if (const char* why = lds_launch_refusal(N, lds, A.max_ops, (size_t)h->lds_per_cu)) return fail(h, VQE_EINVAL, why);
  const bool noisy = A.noise.p1 > 0.0 || A.noise.p2 > 0.0;
  void (*const kernel)(BatchArgs, SpsaArgs) = noisy ? k_lds_minimize_spsa<N, true> : k_lds_minimize_spsa<N, false>;
  const void* fn = (const void*)kernel;
  HIP_TRY(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  {   // the unit loop addresses the state region absolutely (unit_lds_read): the dynamic LDS must start at 0
    hipFuncAttributes fa;
    HIP_TRY(h, hipFuncGetAttributes(&fa, fn));
    if (fa.sharedSizeBytes != 0) return fail(h, VQE_ESTATE, "LDS-resident kernel was built with static LDS");
  }
  HIP_TRY(h, h->spsa_work.reserve((size_t)A.batch * spsa_work_doubles(A.max_params)));
  VQE_TRY(upload(h, h->spsa_opts, &o, 1));
  HIP_TRY(h, hipStreamSynchronize(h->stream));      // (the caller's options go out of scope)
  const SpsaArgs S{h->spsa_opts.p, h->spsa_work.p};
  h->last_pairs = h->last_singles = 0;
  h->last_lds = lds;
  h->last_wg_per_cu = std::max(1, std::min(8, (int)(h->lds_per_cu / lds)));
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  hipLaunchKernelGGL(kernel, dim3(A.batch), dim3(Geo<N>::NT), lds, h->stream, A, S);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  return VQE_OK;
}

// o: options that passed spsa_check
int run_spsa(vqe_t* h, bool env_step, const SpsaOpts& o) {
  HIP_TRY(h, hipSetDevice(h->dev));
  BatchArgs A = make_args(h);
  const int evals = 2 * o.maxiter + 1;      // ids eval_base .. eval_base + 2K; the rows of the trace
  A.maxfun = evals;
  if (env_step) set_env_step(h, A);
  {   // the launch's own refusal, before the trace and the info of the previous run are given up
    const size_t lds = spsa_lds_bytes(h->n, A.max_ops, A.max_params, A.ham.n_groups, A.max_pair);
    if (const char* why = lds_launch_refusal(h->n, lds, A.max_ops, (size_t)h->lds_per_cu)) return fail(h, VQE_EINVAL, why);
  }
  if (h->trace_on) VQE_TRY(arm_trace(h, A, evals));
  h->last_run_dm = false;
  h->lb_batch = 0;
  h->qj_traj_batch = 0;
  VQE_TRY(dispatch_n(h, "the device Adam-SPSA serves n_qubits <= 13 (LDS-resident path) only",
                     [&](auto n) -> int { return launch_spsa<decltype(n)::value>(h, A, o); }, LdsSizes{}));
  h->noise.eval_base += (uint64_t)evals;
  return VQE_OK;
}

}  // namespace

// =========================================================================================
extern "C" {

int vqe_create(int n_qubits, int device_id, vqe_t** out) {
  if (!out) return fail(nullptr, VQE_EINVAL, "out is NULL");
  *out = nullptr;
  if (n_qubits < 1 || n_qubits > 30) return fail(nullptr, VQE_EINVAL, "n_qubits must be in [1, 30]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, VQE_ENODEV, "no HIP device available (the VQE engine has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, VQE_EINVAL, "device_id out of range");
  vqe_t* h = new (std::nothrow) vqe_t;
  if (!h) return fail(nullptr, VQE_ENOMEM, "out of host memory");
  h->n = n_qubits;
  h->dev = device_id;
  h->lds_path = n_qubits <= 13;
  hipDeviceProp_t prop;
  if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&prop, device_id) != hipSuccess ||
      hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
    delete h;
    return fail(nullptr, VQE_EHIP, "HIP device initialisation failed");
  }
  h->stream = h->own_stream;
  h->cu_count = prop.multiProcessorCount;
  h->lds_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
  if (h->lds_per_cu <= 0) h->lds_per_cu = 65536;
  if (h->d_dbg.reserve(8) != hipSuccess || hipMemset(h->d_dbg.p, 0, 64) != hipSuccess) {
    delete h;
    return fail(nullptr, VQE_ENOMEM, "device allocation failed");
  }
  *out = h;
  int rc = vqe_set_init_state(h, nullptr);
  if (rc) { g_create_error = h->err; vqe_destroy(h); *out = nullptr; return rc; }
  return VQE_OK;
}

void vqe_destroy(vqe_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->dev);
  (void)hipStreamSynchronize(h->stream);
  if (h->comm) (void)vqe_comm_destroy(h);
  if (h->dm_ev0) (void)hipEventDestroy(h->dm_ev0);
  if (h->dm_ev1) (void)hipEventDestroy(h->dm_ev1);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
}

const char* vqe_last_error(const vqe_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int vqe_set_stream(vqe_t* h, void* s) {
  if (!h) return VQE_EINVAL;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->stream = s ? (hipStream_t)s : h->own_stream;
  return VQE_OK;
}

int vqe_get_stream(vqe_t* h, void** hip_stream) {
  if (!h || !hip_stream) return VQE_EINVAL;
  *hip_stream = (void*)h->stream;
  return VQE_OK;
}

int vqe_sync(vqe_t* h) {
  if (!h) return VQE_EINVAL;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_device_info(vqe_t* h, int64_t info[4]) {
  if (!h || !info) return VQE_EINVAL;
  info[0] = h->cu_count; info[1] = h->lds_per_cu; info[2] = h->last_wg_per_cu; info[3] = h->lds_path;
  return VQE_OK;
}

int vqe_set_init_state(vqe_t* h, const double* amps) {
  if (!h) return VQE_EINVAL;
  HIP_TRY(h, hipSetDevice(h->dev));
  const size_t dim = (size_t)1 << h->n;
  HIP_TRY(h, h->init.reserve(dim));
  if (amps) {
    HIP_TRY(h, hipMemcpyAsync(h->init.p, amps, dim * 16, hipMemcpyHostToDevice, h->stream));
  } else {
    const double one[2] = {1.0, 0.0};
    HIP_TRY(h, hipMemsetAsync(h->init.p, 0, dim * 16, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->init.p, one, 16, hipMemcpyHostToDevice, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_set_init_state_dev(vqe_t* h, const void* dev_amps) {
  if (!h || !dev_amps) return VQE_EINVAL;
  HIP_TRY(h, hipSetDevice(h->dev));
  const size_t dim = (size_t)1 << h->n;
  HIP_TRY(h, h->init.reserve(dim));
  HIP_TRY(h, hipMemcpyAsync(h->init.p, dev_amps, dim * 16, hipMemcpyDeviceToDevice, h->stream));
  return VQE_OK;
}

int vqe_get_state_dev(vqe_t* h, const double* theta, void* dev_amps) {
  if (!h) return VQE_EINVAL;
  if (!dev_amps || (h->circ_params > 0 && !theta)) return fail(h, VQE_EINVAL, "bad arguments");
  VQE_TRY(kraus_refusal(h, true, true));
  HIP_TRY(h, hipSetDevice(h->dev));
  int rc = load_single(h, 1, theta);
  if (rc) return rc;
  const size_t dim = (size_t)1 << h->n;
  HIP_TRY(h, h->d_state.reserve(dim));
  if ((rc = run(h, Run::State, 0, 0, 0))) return rc;
  HIP_TRY(h, hipMemcpyAsync(dev_amps, h->d_state.p, dim * 16, hipMemcpyDeviceToDevice, h->stream));
  return VQE_OK;
}

int vqe_set_hamiltonian_pauli(vqe_t* h, int n_terms, const uint64_t* xmask, const uint64_t* zmask,
                              const double* coeff) {
  if (!h) return VQE_EINVAL;
  if (n_terms < 0 || (n_terms > 0 && (!xmask || !zmask || !coeff)))
    return fail(h, VQE_EINVAL, "bad Hamiltonian arguments");
  HIP_TRY(h, hipSetDevice(h->dev));
  HamHost H;      // grouped apart from the handle: ham_from_paulis stops at the first bad mask, with H half written
  if (!ham_from_paulis(h->n, n_terms, xmask, zmask, coeff, H))
    return fail(h, VQE_EINVAL, "Pauli mask uses a qubit >= n_qubits");
  return build_hamiltonian(h, &H, h->shard_rank, h->shard_world);
}

int vqe_set_hamiltonian_dense(vqe_t* h, const double* op_re_im, double tol) {
  if (!h) return VQE_EINVAL;
  if (!op_re_im || !(tol >= 0.0)) return fail(h, VQE_EINVAL, "bad Hamiltonian arguments");
  if (h->n > 13) return fail(h, VQE_EINVAL, "a dense 2^n x 2^n operator is accepted up to 13 qubits (17 TB at n = 20): use vqe_set_hamiltonian_pauli");
  // H = sum_{x,z} c(x,z) P(x,z), P|i> = i^{#Y} (-1)^{popc(i & z)} |i ^ x>  =>  for fixed x the coefficients are the
  // Walsh-Hadamard transform over i of the generalised diagonal H[i ^ x, i], divided by 2^n i^{#Y}
  const size_t dim = (size_t)1 << h->n;
  std::vector<uint64_t> xs, zs;
  std::vector<double> cs;
  std::vector<double> re(dim), im(dim);
  double scale = 0.0;
  for (size_t k = 0; k < 2 * dim * dim; ++k) scale = std::max(scale, std::fabs(op_re_im[k]));
  const double cut = tol * (scale > 0 ? scale : 1.0);
  for (size_t x = 0; x < dim; ++x) {
    bool any = false;
    for (size_t i = 0; i < dim; ++i) {
      const double* e = op_re_im + 2 * ((i ^ x) * dim + i);
      re[i] = e[0]; im[i] = e[1];
      any = any || e[0] != 0.0 || e[1] != 0.0;
    }
    if (!any) continue;
    for (size_t step = 1; step < dim; step <<= 1)
      for (size_t i = 0; i < dim; i += 2 * step)
        for (size_t j = i; j < i + step; ++j) {
          const double ar = re[j], ai = im[j], br = re[j + step], bi = im[j + step];
          re[j] = ar + br; im[j] = ai + bi; re[j + step] = ar - br; im[j + step] = ai - bi;
        }
    for (size_t z = 0; z < dim; ++z) {
      double cr = re[z] / (double)dim, ci = im[z] / (double)dim;
      const int ny = __builtin_popcountll(x & z) & 3;      // divide by i^ny
      double vr, vi;
      if (ny == 0) { vr = cr; vi = ci; } else if (ny == 1) { vr = ci; vi = -cr; } else if (ny == 2) { vr = -cr; vi = -ci; } else { vr = -ci; vi = cr; }
      if (std::fabs(vr) <= cut && std::fabs(vi) <= cut) continue;
      if (std::fabs(vi) > 1e-9 * (scale > 0 ? scale : 1.0) && std::fabs(vi) > cut)
        return fail(h, VQE_EINVAL, "operator is not Hermitian (complex Pauli coefficient)");
      xs.push_back(x); zs.push_back(z); cs.push_back(vr);
    }
  }
  return vqe_set_hamiltonian_pauli(h, (int)cs.size(), xs.data(), zs.data(), cs.data());
}

int vqe_hamiltonian_terms(vqe_t* h, int32_t* n_terms, int32_t* n_xgroups) {
  if (!h || !n_terms || !n_xgroups) return VQE_EINVAL;
  if (!h->ham_set) return fail(h, VQE_ESTATE, "no Hamiltonian set");
  *n_terms = (int32_t)h->ham_host.hx.size();
  *n_xgroups = (int32_t)h->ham_host.gx_all.size();
  return VQE_OK;
}

// ---- RCCL behind the C ABI ----------------------------------------------------------------------------------------
// The collective of the term-sharded expectation sum as a library call: one ncclAllReduce(SUM, float64, count = batch) of
// the handle's energy array, in place, on the handle's stream.  librccl is opened lazily (no link-time dependency: a
// process that never shards never loads it; under PyTorch the already-loaded copy of the same SONAME is reused).
extern "C++" {      // (helpers with C++ types inside the C-ABI block)
namespace {
struct Id128 { char b[128]; };      // ncclUniqueId, passed by value
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id128, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
Rccl& rccl() {
  static Rccl r;
  if (!r.lib) {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.lib) break;
    }
    if (r.lib) {
      r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.lib, "ncclGetUniqueId");
      r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.lib, "ncclCommInitRank");
      r.AllReduce = (decltype(r.AllReduce))dlsym(r.lib, "ncclAllReduce");
      r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
      r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
      r.ok = r.GetUniqueId && r.CommInitRank && r.AllReduce && r.CommDestroy;
    }
  }
  return r;
}
}  // namespace
}  // extern "C++"

int vqe_comm_unique_id(void* id128) {
  if (!id128) return VQE_EINVAL;
  Rccl& r = rccl();
  if (!r.ok) return fail(nullptr, VQE_ENODEV, "librccl not found");
  const int rc = r.GetUniqueId(id128);
  return rc ? fail(nullptr, VQE_EHIP, std::string("ncclGetUniqueId: ") + (r.GetErrorString ? r.GetErrorString(rc) : "error")) : VQE_OK;
}

int vqe_comm_init(vqe_t* h, int rank, int world, const void* id128) {
  if (!h || !id128) return VQE_EINVAL;
  if (world < 1 || rank < 0 || rank >= world) return fail(h, VQE_EINVAL, "bad rank / world");
  if (h->comm) return fail(h, VQE_ESTATE, "communicator exists already (vqe_comm_destroy first)");
  Rccl& r = rccl();
  if (!r.ok) return fail(h, VQE_ENODEV, "librccl not found");
  HIP_TRY(h, hipSetDevice(h->dev));
  Id128 id;
  std::memcpy(id.b, id128, 128);
  void* comm = nullptr;
  const int rc = r.CommInitRank(&comm, world, id, rank);
  if (rc) return fail(h, VQE_EHIP, std::string("ncclCommInitRank: ") + (r.GetErrorString ? r.GetErrorString(rc) : "error"));
  h->comm = comm;
  h->comm_world = world;
  return VQE_OK;
}

int vqe_comm_allreduce_energy(vqe_t* h) {
  if (!h) return VQE_EINVAL;
  if (!h->comm) return fail(h, VQE_ESTATE, "vqe_comm_init has not been called");
  if (h->batch <= 0) return fail(h, VQE_ESTATE, "no batch loaded");
  Rccl& r = rccl();
  const int rc = r.AllReduce(h->d_f.p, h->d_f.p, (size_t)h->batch, /* ncclFloat64 */ 8, /* ncclSum */ 0, h->comm, h->stream);
  return rc ? fail(h, VQE_EHIP, std::string("ncclAllReduce: ") + (r.GetErrorString ? r.GetErrorString(rc) : "error")) : VQE_OK;
}

int vqe_comm_destroy(vqe_t* h) {
  if (!h) return VQE_EINVAL;
  if (h->comm) {
    (void)hipStreamSynchronize(h->stream);
    (void)rccl().CommDestroy(h->comm);
    h->comm = nullptr;
    h->comm_world = 0;
  }
  return VQE_OK;
}

int vqe_hamiltonian_layout(vqe_t* h, int32_t out[4]) {
  if (!h || !out) return VQE_EINVAL;
  if (!h->ham_set) return fail(h, VQE_ESTATE, "no Hamiltonian set");
  out[0] = h->ham.n_groups; out[1] = h->ham.n_units; out[2] = h->ham.n_cls; out[3] = h->ham.has_diag;
  return VQE_OK;
}

int vqe_cobyla_placement(int n_qubits, int max_ops, int max_pair, int max_params, int n_groups, int n_params, int wide,
                         int64_t out[8]) {
  if (!out || n_qubits < 1 || n_qubits > 13 || max_ops < 1 || max_pair < 0 || max_pair > max_ops || max_params < 1 ||
      n_groups < 0 || n_params < 1 || n_params > max_params)
    return VQE_EINVAL;
  if (wide && !(n_qubits >= kWideMinN && max_params > 64)) return VQE_EINVAL;      // no launch takes the WIDE variant there
  report_placement(n_qubits, max_ops, max_pair, max_params, n_groups, n_params, wide != 0, (size_t)160 * 1024, out);
  return VQE_OK;
}

int vqe_batch_cobyla_placement(vqe_t* h, int circuit, int64_t out[8]) {
  if (!h || !out) return VQE_EINVAL;
  if (!h->lds_path) return fail(h, VQE_EINVAL, "n_qubits outside the LDS-resident range");
  if (!h->ham_set) return fail(h, VQE_ESTATE, "no Hamiltonian set");
  if (circuit < 0 || circuit >= h->batch) return fail(h, VQE_EINVAL, "circuit index out of range");
  if (h->h_par_count[circuit] < 1) return fail(h, VQE_EINVAL, "the circuit has no parameters: the optimiser does not run");
  report_placement(h->n, h->max_ops, h->max_pair, h->max_params, h->ham.n_groups, h->h_par_count[circuit],
                   wide_launch(h->n, h->max_params), (size_t)h->lds_per_cu, out);
  return VQE_OK;
}

int vqe_unit_bank_score(vqe_t* h, double out[4]) {
  if (!h || !out) return VQE_EINVAL;
  if (!h->ham_set) return fail(h, VQE_ESTATE, "no Hamiltonian set");
  for (int i = 0; i < 4; ++i) out[i] = h->unit_score[i];
  return VQE_OK;
}

int vqe_set_term_shard(vqe_t* h, int rank, int world) {
  if (!h) return VQE_EINVAL;
  if (world < 1 || rank < 0 || rank >= world) return fail(h, VQE_EINVAL, "bad shard rank/world");
  if (h->ham_set) { HIP_TRY(h, hipSetDevice(h->dev)); return build_hamiltonian(h, nullptr, rank, world); }
  h->shard_rank = rank;
  h->shard_world = world;
  return VQE_OK;
}

int vqe_set_amplitude_shard(vqe_t* h, int rank, int world) {
  if (!h) return VQE_EINVAL;
  if (world < 1 || rank < 0 || rank >= world) return fail(h, VQE_EINVAL, "bad shard rank/world");
  if (h->lds_path && world > 1)
    return fail(h, VQE_ESTATE, "amplitude sharding of the energy sweep exists on the streaming path (n >= 14); use vqe_set_term_shard");
  if (world > 1 && (h->pauli_tab.has1 || h->pauli_tab.has2))
    return fail(h, VQE_ESTATE, "Pauli channel tables (vqe_set_noise_pauli) take no amplitude-sharded handle: remove them first");
  const size_t blocks = ((size_t)1 << h->n) >> kETileBits;     // tiles of the energy sweep (vqe_tile.h)
  if (!h->lds_path && (blocks % (size_t)world) != 0) return fail(h, VQE_EINVAL, "world must divide the number of sweep tiles of the energy reduction");
  h->amp_rank = rank;
  h->amp_world = world;
  ++h->gen;
  return VQE_OK;
}

int vqe_set_stream_grad(vqe_t* h, int enable) {
  if (!h) return VQE_EINVAL;
  h->stream_grad = enable != 0;      // (n <= 13: the LDS-resident kernel serves every gradient; nothing to switch)
  return VQE_OK;
}

int vqe_set_env_pairing(vqe_t* h, int enable) {
  if (!h) return VQE_EINVAL;
  h->env_pairing = enable != 0;
  return VQE_OK;
}

int vqe_last_env_pairing(vqe_t* h, int64_t out[4]) {
  if (!h || !out) return VQE_EINVAL;
  out[0] = h->last_pairs > 0 || h->last_singles > 0;
  out[1] = h->last_pairs;
  out[2] = h->last_singles;
  out[3] = (int64_t)h->last_lds;
  return VQE_OK;
}

int vqe_pair_lds_plan(int n_qubits, int max_ops, int max_pair, int max_params, int n_groups, int64_t out[12]) {
  if (!out || n_qubits < 10 || n_qubits > 13 || max_ops < 1 || max_pair < 0 || max_pair > max_ops || max_params < 1 || n_groups < 0)
    return VQE_EINVAL;
  const PairLdsPlan p = pair_lds_plan(n_qubits, max_ops, max_params, n_groups, max_pair);
  out[0] = (int64_t)p.sched; out[1] = (int64_t)p.lay; out[2] = (int64_t)p.cs; out[3] = (int64_t)p.xm;
  out[4] = (int64_t)p.zm; out[5] = (int64_t)p.meta; out[6] = (int64_t)p.sb; out[7] = (int64_t)p.sidx;
  out[8] = (int64_t)p.rec; out[9] = (int64_t)p.bytes;
  out[10] = (int64_t)lds_bytes(n_qubits, max_ops, max_params, n_groups, max_pair, false);   // the single launch
  out[11] = (int64_t)((size_t)16 << n_qubits);      // the state region: [0, out[11])
  return VQE_OK;
}

int vqe_set_stream_lbfgs(vqe_t* h, int enable) {
  if (!h) return VQE_EINVAL;
  h->stream_lbfgs = enable != 0;     // (n <= 13: k_lds_minimize_lbfgs serves every run; nothing to switch)
  return VQE_OK;
}

int vqe_set_noise(vqe_t* h, double p1, double p2, uint64_t seed) {
  if (!h) return VQE_EINVAL;
  if (!(p1 >= 0.0 && p1 <= 1.0 && p2 >= 0.0 && p2 <= 1.0)) return fail(h, VQE_EINVAL, "noise probability outside [0,1]");
  h->noise = NoiseCfg{p1, p2, seed, 0ull, h->noise.shot_sigma};
  ++h->gen;
  ++h->qj_ver;
  return VQE_OK;
}

int vqe_set_noise_mode(vqe_t* h, int mode) {
  if (!h) return VQE_EINVAL;
  if (mode != 0 && mode != 1) return fail(h, VQE_EINVAL, "noise mode: 0 (Pauli trajectories) or 1 (exact channel)");
  if (mode == 1 && (h->n < 2 || h->n > 13)) return fail(h, VQE_EINVAL, "the exact channel mode (density matrix) serves 2 <= n_qubits <= 13");
  h->noise_mode = mode;
  return VQE_OK;
}

int vqe_set_dm_batched(vqe_t* h, int max_resident) {
  if (!h) return VQE_EINVAL;
  if (max_resident < -1) return fail(h, VQE_EINVAL, "max_resident: 0 (serial path), -1 (a quarter of the free device memory) or R >= 1");
  h->dm_batched = max_resident;
  h->dm_auto_cap = 0;
  return VQE_OK;
}

int vqe_set_dm_grad(vqe_t* h, int enable) {
  if (!h) return VQE_EINVAL;
  h->dm_grad = enable != 0;      // (takes effect in noise mode 1 with vqe_set_dm_batched != 0; elsewhere nothing to switch)
  return VQE_OK;
}

int vqe_set_noise_kraus(vqe_t* h, int n1, const double* K1, int n2, const double* K2) {
  if (!h) return VQE_EINVAL;
  if (n1 < 0 || n1 > 16 || n2 < 0 || n2 > 64) return fail(h, VQE_EINVAL, "Kraus operators per slot: 0 <= n1 <= 16, 0 <= n2 <= 64");
  if ((n1 > 0 && !K1) || (n2 > 0 && !K2)) return fail(h, VQE_EINVAL, "Kraus array is NULL");
  DmKraus k;
  k.n1 = n1;
  k.n2 = n2;
  for (int i = 0; i < n1 * 4; ++i) k.K1.push_back(cplx(K1[2 * i], K1[2 * i + 1]));
  for (int i = 0; i < n2 * 16; ++i) k.K2.push_back(cplx(K2[2 * i], K2[2 * i + 1]));
  // (a NaN fails both comparisons)
  if ((n1 > 0 && !(kraus_tp_defect(k.K1.data(), n1, 2) <= 1e-12)) || (n2 > 0 && !(kraus_tp_defect(k.K2.data(), n2, 4) <= 1e-12)))
    return fail(h, VQE_EINVAL, "Kraus set is not trace preserving: max |sum K^+ K - I| > 1e-12");
  h->kraus = std::move(k);
  set_channels(h);
  ++h->gen;      // the plans and channel tables of the resident batch are made again
  ++h->qj_ver;
  return VQE_OK;
}

int vqe_set_kraus_traj(vqe_t* h, int n_traj) {
  if (!h) return VQE_EINVAL;
  if (n_traj < 0 || n_traj > 4096) return fail(h, VQE_EINVAL, "trajectories per evaluation: 0 (off) or 1 .. 4096");
  if (n_traj != h->kraus_traj) h->qj_traj_batch = 0;      // (vqe_batch_fetch_traj hands out batch x n_traj of the run that made them)
  h->kraus_traj = n_traj;
  return VQE_OK;
}

int vqe_set_stream_kraus_traj(vqe_t* h, int max_resident) {
  if (!h) return VQE_EINVAL;
  if (max_resident < -1) return fail(h, VQE_EINVAL, "max_resident: 0 (off), -1 (a quarter of the free device memory) or R >= 1");
  h->sq_resident = max_resident;      // (n <= 13: the LDS-resident kernel serves every trajectory; nothing to switch)
  h->sq_auto_cap = 0;
  return VQE_OK;
}

int vqe_stream_kraus_traj_info(vqe_t* h, int64_t out[4]) {
  if (!h || !out) return VQE_EINVAL;
  std::copy(h->sq_info, h->sq_info + 4, out);
  return VQE_OK;
}

int vqe_kraus_traj_info(vqe_t* h, int64_t out[4]) {
  if (!h || !out) return VQE_EINVAL;
  if (h->qj_jsum_batch > 0) {      // the jump sums of the last evaluation wait on the device
    HIP_TRY(h, hipSetDevice(h->dev));
    std::vector<long long> js((size_t)h->qj_jsum_batch);
    HIP_TRY(h, hipMemcpyAsync(js.data(), h->qj_jsum.p, js.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->qj_info[2] = 0;
    for (long long j : js) h->qj_info[2] += j;
    h->qj_jsum_batch = 0;
  }
  out[0] = h->kraus_traj;
  std::copy(h->qj_info + 1, h->qj_info + 4, out + 1);
  return VQE_OK;
}

int vqe_batch_fetch_traj(vqe_t* h, double* e) {
  if (!h) return VQE_EINVAL;
  if (!e) return fail(h, VQE_EINVAL, "e is NULL");
  if (h->qj_traj_batch <= 0 || h->qj_traj_batch != h->batch)
    return fail(h, VQE_ESTATE, "no per-trajectory energies: the last run was no trajectory energy run or env-step (vqe_set_kraus_traj)");
  HIP_TRY(h, hipSetDevice(h->dev));
  HIP_TRY(h, hipMemcpyAsync(e, h->qj_e.p, (size_t)h->batch * (size_t)h->qj_info[0] * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_noise_kraus_info(vqe_t* h, int32_t out[2]) {
  if (!h || !out) return VQE_EINVAL;
  out[0] = h->kraus.n1;
  out[1] = h->kraus.n2;
  return VQE_OK;
}

int vqe_set_noise_pauli(vqe_t* h, const double* w1, const double* w2) {
  if (!h) return VQE_EINVAL;
  if (h->amp_world > 1) return fail(h, VQE_ESTATE, "Pauli channel tables (vqe_set_noise_pauli) take no amplitude-sharded handle");
  if ((w1 && !pauli_weights_ok(w1, 3)) || (w2 && !pauli_weights_ok(w2, 15)))
    return fail(h, VQE_EINVAL, "Pauli channel table: every weight a number in [0, 1], their sum at most 1");
  NoisePauliTab t{};
  if (w1) { t.has1 = 1; pauli_cumulate(w1, 3, t.cum1); }
  if (w2) { t.has2 = 1; pauli_cumulate(w2, 15, t.cum2); }
  if (w1 || w2) {
    // (in stream order behind the launches that read the old table; the source lives in this frame)
    HIP_TRY(h, hipSetDevice(h->dev));
    HIP_TRY(h, h->d_pauli_tab.reserve(1));
    HIP_TRY(h, hipMemcpyAsync(h->d_pauli_tab.p, &t, sizeof t, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  h->pauli_tab = t;
  std::fill(h->pauli_w1, h->pauli_w1 + 3, 0.0);
  std::fill(h->pauli_w2, h->pauli_w2 + 15, 0.0);
  if (w1) std::copy(w1, w1 + 3, h->pauli_w1);
  if (w2) std::copy(w2, w2 + 15, h->pauli_w2);
  set_channels(h);
  ++h->gen;      // the plans and channel tables of the resident batch are made again
  ++h->qj_ver;
  return VQE_OK;
}

int vqe_set_noise_grad(vqe_t* h, int n_real, int hold) {
  if (!h) return VQE_EINVAL;
  if (n_real < 0 || n_real > kNoiseGradMaxReal) return fail(h, VQE_EINVAL, "vqe_set_noise_grad: n_real must be in [0, 4096]");
  if (h->amp_world > 1) return fail(h, VQE_ESTATE, "gradients of frozen noise realisations (vqe_set_noise_grad) take no amplitude-sharded handle");
  h->noise_grad_T = n_real;
  h->noise_grad_hold = hold != 0;
  return VQE_OK;
}

int vqe_set_stream_noise_grad(vqe_t* h, int max_resident) {
  if (!h) return VQE_EINVAL;
  if (max_resident < -1) return fail(h, VQE_EINVAL, "max_resident: 0 (off), -1 (a quarter of the free device memory) or R >= 1");
  if (h->amp_world > 1) return fail(h, VQE_ESTATE, "gradients of frozen noise realisations (vqe_set_stream_noise_grad) take no amplitude-sharded handle");
  h->sng_resident = max_resident;      // (n <= 13: the LDS-resident kernel serves every noisy gradient; nothing to switch)
  h->sng_auto_cap = 0;
  return VQE_OK;
}

int vqe_stream_noise_grad_info(vqe_t* h, int64_t out[4]) {
  if (!h || !out) return VQE_EINVAL;
  out[0] = h->sng_resident;
  std::copy(h->sng_info + 1, h->sng_info + 4, out + 1);
  return VQE_OK;
}

int vqe_noise_grad_advance(vqe_t* h) {
  if (!h) return VQE_EINVAL;
  h->noise.eval_base += (uint64_t)h->noise_grad_T;
  return VQE_OK;
}

int vqe_noise_grad_info(vqe_t* h, int64_t out[4]) {
  if (!h || !out) return VQE_EINVAL;
  out[0] = h->noise_grad_T;
  out[1] = h->noise_grad_hold ? 1 : 0;
  out[2] = (int64_t)h->noise.eval_base;
  out[3] = 0;
  return VQE_OK;
}

int vqe_noise_pauli_info(vqe_t* h, int32_t out[2]) {
  if (!h || !out) return VQE_EINVAL;
  out[0] = h->pauli_tab.has1;
  out[1] = h->pauli_tab.has2;
  return VQE_OK;
}

int vqe_set_dm_rot2(vqe_t* h, int enable) {
  if (!h) return VQE_EINVAL;
  if (h->dm_rot2 != (enable != 0)) ++h->gen;      // (takes effect in noise mode 1: a two-qubit rotation is then a member of the plans)
  h->dm_rot2 = enable != 0;
  return VQE_OK;
}

int vqe_dm_batch_info(vqe_t* h, int64_t out[4]) {
  if (!h || !out) return VQE_EINVAL;
  std::copy(h->dm_info, h->dm_info + 4, out);
  return VQE_OK;
}

int vqe_dm_plan(int n_qubits, int n_gates, const int32_t* kind, const int32_t* q0, const int32_t* q1, const int32_t* pidx,
                const double* theta, double p1, double p2, int cap_blocks, int32_t* n_blocks, int32_t* windows, double* S) {
  if (n_qubits < 2 || n_gates < 0 || !n_blocks || (n_gates > 0 && (!kind || !q0 || !q1 || !pidx))) return VQE_EINVAL;
  std::vector<GateRec> g((size_t)n_gates);
  for (int i = 0; i < n_gates; ++i) {
    if (kind[i] < 0 || kind[i] > VQE_GATE_DEPOL2 || q0[i] < 0 || q0[i] >= n_qubits) return VQE_EINVAL;
    const bool two = kind[i] == VQE_GATE_CNOT || kind[i] == VQE_GATE_DEPOL2;
    if (two && (q1[i] < 0 || q1[i] >= n_qubits || q1[i] == q0[i])) return VQE_EINVAL;
    if (kind[i] >= VQE_GATE_RX && kind[i] <= VQE_GATE_RZ && (pidx[i] < 0 || !theta)) return VQE_EINVAL;
    g[i] = GateRec{kind[i], q0[i], q1[i], pidx[i]};
  }
  std::vector<DmBlockHost> blocks;
  dm_make_blocks(n_qubits, g.data(), n_gates, theta, p1, p2, blocks);
  *n_blocks = (int32_t)blocks.size();
  if (!windows || !S) return VQE_OK;
  if ((int)blocks.size() > cap_blocks) return VQE_EINVAL;
  for (size_t k = 0; k < blocks.size(); ++k) {
    windows[2 * k] = blocks[k].a;
    windows[2 * k + 1] = blocks[k].b;
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
      S[k * 512 + r * 16 + c] = blocks[k].S.m[r][c].real();
      S[k * 512 + 256 + r * 16 + c] = blocks[k].S.m[r][c].imag();
    }
  }
  return VQE_OK;
}

int vqe_noise_mode_info(vqe_t* h, int32_t out[2]) {
  if (!h || !out) return VQE_EINVAL;
  out[0] = h->noise_mode;
  out[1] = h->dm_blocks_last;
  return VQE_OK;
}

int vqe_set_shot_noise(vqe_t* h, double sigma_total, uint64_t seed) {
  if (!h) return VQE_EINVAL;
  if (!(sigma_total >= 0.0)) return fail(h, VQE_EINVAL, "sigma_total must be >= 0");
  h->noise.shot_sigma = sigma_total;
  h->noise.seed = seed;
  return VQE_OK;
}

int vqe_set_circuit(vqe_t* h, int n_gates, const int32_t* kind, const int32_t* q0, const int32_t* q1,
                    const int32_t* pidx, int n_params) {
  if (!h) return VQE_EINVAL;
  if (n_gates < 0 || n_params < 0 || (n_gates > 0 && (!kind || !q0 || !q1 || !pidx)))
    return fail(h, VQE_EINVAL, "bad circuit arguments");
  int rc = check_gates(h, n_gates, kind, q0, q1, pidx, n_params);
  if (rc) return rc;
  h->circ.resize(n_gates);
  for (int i = 0; i < n_gates; ++i) h->circ[i] = GateRec{kind[i], q0[i], q1[i], pidx[i]};
  h->circ_params = n_params;
  return VQE_OK;
}

int vqe_energy_batch(vqe_t* h, int batch, const double* theta, double* energy) {
  if (!h) return VQE_EINVAL;
  if (batch < 1 || !energy || (h->circ_params > 0 && !theta)) return fail(h, VQE_EINVAL, "bad arguments");
  VQE_TRY(kraus_refusal(h, false, true));
  HIP_TRY(h, hipSetDevice(h->dev));
  int rc = load_single(h, batch, theta);
  if (rc) return rc;
  if ((rc = ready(h))) return rc;
  if ((rc = run(h, Run::Energy, 0, 0, 0))) return rc;
  HIP_TRY(h, hipMemcpyAsync(energy, h->d_f.p, (size_t)batch * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_energy(vqe_t* h, const double* theta, double* energy) { return vqe_energy_batch(h, 1, theta, energy); }

int vqe_get_state(vqe_t* h, const double* theta, double* amps) {
  if (!h) return VQE_EINVAL;
  if (!amps || (h->circ_params > 0 && !theta)) return fail(h, VQE_EINVAL, "bad arguments");
  VQE_TRY(kraus_refusal(h, true, true));
  HIP_TRY(h, hipSetDevice(h->dev));
  int rc = load_single(h, 1, theta);
  if (rc) return rc;
  const size_t dim = (size_t)1 << h->n;
  HIP_TRY(h, h->d_state.reserve(dim));
  if ((rc = run(h, Run::State, 0, 0, 0))) return rc;
  HIP_TRY(h, hipMemcpyAsync(amps, h->d_state.p, dim * 16, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_minimize_cobyla(vqe_t* h, const double* x0, double rhobeg, double rhoend, int maxfun, double* x,
                        double* f, int32_t* nfev) {
  if (!h) return VQE_EINVAL;
  if (maxfun < 1 || !(rhobeg > 0) || !(rhoend > 0)) return fail(h, VQE_EINVAL, "bad COBYLA arguments");
  if (h->circ_params > 0 && (!x0 || !x)) return fail(h, VQE_EINVAL, "x0/x is NULL");
  VQE_TRY(kraus_refusal(h, false, true));
  HIP_TRY(h, hipSetDevice(h->dev));
  int rc = load_single(h, 1, x0);
  if (rc) return rc;
  if ((rc = ready(h))) return rc;
  if ((rc = run(h, Run::Minimize, rhobeg, rhoend, maxfun))) return rc;
  return vqe_batch_fetch(h, x, f, nfev);
}

int vqe_batch_load(vqe_t* h, int batch, const int64_t* gate_off, const int32_t* kind, const int32_t* q0,
                   const int32_t* q1, const int32_t* pidx, const int64_t* par_off, const double* theta0) {
  if (!h) return VQE_EINVAL;
  if (batch < 1 || !gate_off || !par_off) return fail(h, VQE_EINVAL, "bad batch arguments");
  HIP_TRY(h, hipSetDevice(h->dev));
  const int64_t G = gate_off[batch], PT = par_off[batch];
  if (gate_off[0] != 0 || par_off[0] != 0 || G < 0 || PT < 0) return fail(h, VQE_EINVAL, "offsets must start at 0");
  if ((G > 0 && (!kind || !q0 || !q1 || !pidx)) || (PT > 0 && !theta0)) return fail(h, VQE_EINVAL, "NULL array");
  std::vector<GateRec> gates((size_t)G);
  std::vector<int64_t> gbeg(batch), pbeg(batch);
  std::vector<int32_t> gcnt(batch), pcnt(batch);
  for (int b = 0; b < batch; ++b) {
    const int64_t g0 = gate_off[b], g1 = gate_off[b + 1], p0 = par_off[b], p1 = par_off[b + 1];
    if (g1 < g0 || p1 < p0 || g1 > G || p1 > PT) return fail(h, VQE_EINVAL, "offsets not monotone");
    int rc = check_gates(h, g1 - g0, kind + g0, q0 + g0, q1 + g0, pidx + g0, (int)(p1 - p0));
    if (rc) return rc;
    gbeg[b] = g0; gcnt[b] = (int32_t)(g1 - g0); pbeg[b] = p0; pcnt[b] = (int32_t)(p1 - p0);
  }
  for (int64_t i = 0; i < G; ++i) gates[i] = GateRec{kind[i], q0[i], q1[i], pidx[i]};
  return load_batch(h, batch, gates, gbeg, gcnt, pbeg, pcnt, theta0, PT);
}

int vqe_batch_run_energy(vqe_t* h) {
  int rc = ready(h);
  if (rc) return rc;
  return run(h, Run::Energy, 0, 0, 0);
}

int vqe_energy_grad_batch(vqe_t* h, int batch, const double* theta, double* energy, double* grad) {
  if (!h) return VQE_EINVAL;
  if (batch < 1 || !energy || (h->circ_params > 0 && (!theta || !grad))) return fail(h, VQE_EINVAL, "bad arguments");
  int rc;
  if ((rc = grad_refusal(h))) return rc;
  if ((rc = dm_circuit_refusal(h))) return rc;
  HIP_TRY(h, hipSetDevice(h->dev));
  if ((rc = load_single(h, batch, theta))) return rc;
  if ((rc = ready(h))) return rc;
  if ((rc = run_grad(h))) return rc;
  HIP_TRY(h, hipMemcpyAsync(energy, h->d_f.p, (size_t)batch * 8, hipMemcpyDeviceToHost, h->stream));
  if (h->total_params) HIP_TRY(h, hipMemcpyAsync(grad, h->d_grad.p, (size_t)h->total_params * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_batch_run_energy_grad(vqe_t* h) {
  int rc = ready(h);
  if (rc) return rc;
  return run_grad(h);
}

int vqe_batch_fetch_grad(vqe_t* h, double* grad) {
  if (!h) return VQE_EINVAL;
  if (h->batch <= 0) return fail(h, VQE_ESTATE, "no batch loaded");
  if (!grad && h->total_params) return fail(h, VQE_EINVAL, "grad is NULL");
  if (h->d_grad.cap < (size_t)h->total_params + 1) return fail(h, VQE_ESTATE, "vqe_batch_run_energy_grad has not been called");
  HIP_TRY(h, hipSetDevice(h->dev));
  if (h->total_params)
    HIP_TRY(h, hipMemcpyAsync(grad, h->d_grad.p, (size_t)h->total_params * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_batch_run_reduction(vqe_t* h) {
  int rc = ready(h);
  if (rc) return rc;
  return run(h, Run::Reduce, 0, 0, 0);
}

int vqe_batch_run_minimize(vqe_t* h, double rhobeg, double rhoend, int maxfun) {
  int rc = ready(h);
  if (rc) return rc;
  if (maxfun < 1 || !(rhobeg > 0) || !(rhoend > 0)) return fail(h, VQE_EINVAL, "bad COBYLA arguments");
  return run(h, Run::Minimize, rhobeg, rhoend, maxfun);
}

int vqe_batch_set_new_gate(vqe_t* h, const int32_t* new_gate) {
  if (!h) return VQE_EINVAL;
  if (h->batch <= 0) return fail(h, VQE_ESTATE, "no batch loaded");
  if (!new_gate) { h->has_new_gate = false; return VQE_OK; }
  for (int b = 0; b < h->batch; ++b)
    if (new_gate[b] < -1 || new_gate[b] >= h->h_gate_count[b]) return fail(h, VQE_EINVAL, "new_gate index out of range");
  HIP_TRY(h, hipSetDevice(h->dev));
  int rc = upload(h, h->d_new_gate, new_gate, (size_t)h->batch);
  if (rc) return rc;
  h->h_new_gate.assign(new_gate, new_gate + h->batch);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->has_new_gate = true;
  return VQE_OK;
}

int vqe_batch_run_env_step(vqe_t* h, double rhobeg, double rhoend, int maxfun) {
  int rc = ready(h);
  if (rc) return rc;
  if (maxfun < 1 || !(rhobeg > 0) || !(rhoend > 0)) return fail(h, VQE_EINVAL, "bad COBYLA arguments");
  return run(h, Run::EnvStep, rhobeg, rhoend, maxfun);
}

int vqe_lbfgs_default_opts(vqe_lbfgs_opts_t* o) {
  if (!o) return VQE_EINVAL;
  *o = vqe_lbfgs_opts_t{8, 100, 1000, 20, 1e-6, 1e-12, 1e-4};
  return VQE_OK;
}

int vqe_minimize_lbfgs(vqe_t* h, const double* x0, const vqe_lbfgs_opts_t* opts, double* x, double* f, int32_t* nfev,
                       int32_t* nit, int32_t* status) {
  if (!h) return VQE_EINVAL;
  vqe_lbfgs_opts_t o;
  int rc;
  if ((rc = lbfgs_check(h, opts, &o))) return rc;
  if (!f || (h->circ_params > 0 && (!x0 || !x))) return fail(h, VQE_EINVAL, "x0 / x / f is NULL");
  if ((rc = dm_circuit_refusal(h))) return rc;
  HIP_TRY(h, hipSetDevice(h->dev));
  if ((rc = load_single(h, 1, x0))) return rc;
  if ((rc = ready(h))) return rc;
  if ((rc = run_lbfgs(h, false, o))) return rc;
  if ((rc = vqe_batch_fetch(h, x, f, nfev))) return rc;
  return (nit || status) ? vqe_batch_fetch_lbfgs_info(h, nit, status) : VQE_OK;
}

int vqe_batch_run_minimize_lbfgs(vqe_t* h, const vqe_lbfgs_opts_t* opts) {
  if (!h) return VQE_EINVAL;
  vqe_lbfgs_opts_t o;
  int rc;
  if ((rc = lbfgs_check(h, opts, &o))) return rc;
  if ((rc = ready(h))) return rc;
  return run_lbfgs(h, false, o);
}

int vqe_batch_run_env_step_lbfgs(vqe_t* h, const vqe_lbfgs_opts_t* opts) {
  if (!h) return VQE_EINVAL;
  vqe_lbfgs_opts_t o;
  int rc;
  if ((rc = lbfgs_check(h, opts, &o))) return rc;
  if ((rc = ready(h))) return rc;
  return run_lbfgs(h, true, o);
}

int vqe_batch_fetch_lbfgs_info(vqe_t* h, int32_t* nit, int32_t* status) {
  if (!h) return VQE_EINVAL;
  if (h->batch <= 0 || h->lb_batch != h->batch) return fail(h, VQE_ESTATE, "no device L-BFGS run on the resident batch");
  HIP_TRY(h, hipSetDevice(h->dev));
  if (nit) HIP_TRY(h, hipMemcpyAsync(nit, h->lb_nit.p, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
  if (status) HIP_TRY(h, hipMemcpyAsync(status, h->lb_status.p, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_spsa_default_opts(vqe_spsa_opts_t* o) {
  if (!o) return VQE_EINVAL;
  const SpsaOpts d = spsa_default_opts();
  *o = vqe_spsa_opts_t{d.maxiter, d.a, d.alpha, d.stability, d.c, d.gamma, d.beta_1, d.beta_2, d.lamda, d.eps, d.seed};
  return VQE_OK;
}

int vqe_minimize_spsa(vqe_t* h, const double* x0, const vqe_spsa_opts_t* opts, double* x, double* f, int32_t* nfev) {
  if (!h) return VQE_EINVAL;
  SpsaOpts o;
  int rc;
  if ((rc = spsa_check(h, opts, &o))) return rc;
  if (!f || (h->circ_params > 0 && (!x0 || !x))) return fail(h, VQE_EINVAL, "x0 / x / f is NULL");
  HIP_TRY(h, hipSetDevice(h->dev));
  if ((rc = load_single(h, 1, x0))) return rc;
  if ((rc = ready(h))) return rc;
  if ((rc = run_spsa(h, false, o))) return rc;
  return vqe_batch_fetch(h, x, f, nfev);
}

int vqe_batch_run_minimize_spsa(vqe_t* h, const vqe_spsa_opts_t* opts) {
  if (!h) return VQE_EINVAL;
  SpsaOpts o;
  int rc;
  if ((rc = spsa_check(h, opts, &o))) return rc;
  if ((rc = ready(h))) return rc;
  return run_spsa(h, false, o);
}

int vqe_batch_run_env_step_spsa(vqe_t* h, const vqe_spsa_opts_t* opts) {
  if (!h) return VQE_EINVAL;
  SpsaOpts o;
  int rc;
  if ((rc = spsa_check(h, opts, &o))) return rc;
  if ((rc = ready(h))) return rc;
  return run_spsa(h, true, o);
}

int vqe_batch_fetch(vqe_t* h, double* x, double* f, int32_t* nfev) {
  if (!h) return VQE_EINVAL;
  if (h->batch <= 0) return fail(h, VQE_ESTATE, "no batch loaded");
  HIP_TRY(h, hipSetDevice(h->dev));
  if (x && h->total_params)
    HIP_TRY(h, hipMemcpyAsync(x, h->d_x.p, (size_t)h->total_params * 8, hipMemcpyDeviceToHost, h->stream));
  if (f) HIP_TRY(h, hipMemcpyAsync(f, h->d_f.p, (size_t)h->batch * 8, hipMemcpyDeviceToHost, h->stream));
  if (nfev) HIP_TRY(h, hipMemcpyAsync(nfev, h->d_nfev.p, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_batch_fetch_xopt(vqe_t* h, double* x) {
  if (!h) return VQE_EINVAL;
  if (h->batch <= 0) return fail(h, VQE_ESTATE, "no batch loaded");
  if (!x && h->total_params) return fail(h, VQE_EINVAL, "x is NULL");
  HIP_TRY(h, hipSetDevice(h->dev));
  if (h->total_params)
    HIP_TRY(h, hipMemcpyAsync(x, h->d_xraw.p, (size_t)h->total_params * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

// ---- device Lanczos (vqe_lanczos.h) ---------------------------------------------------------------------------------
extern "C++" {
namespace {
// Everything a vqe_lanczos call can be refused for, before anything is launched or given up.
int lanczos_check(vqe_t* h, const vqe_lanczos_opts_t* opts, LzOptions* o) {
  vqe_lanczos_opts_t d;
  vqe_lanczos_default_opts(&d);
  if (opts) d = *opts;
  if (!h->ham_set) return fail(h, VQE_ESTATE, "no Hamiltonian set");
  if (h->shard_world > 1)
    return fail(h, VQE_ESTATE, "vqe_lanczos on a term-sharded handle: a shard's spectrum is not the Hamiltonian's");
  if (h->amp_world > 1) return fail(h, VQE_ESTATE, "vqe_lanczos on an amplitude-sharded handle: it holds a slice of the register");
  if (d.which != 0 && d.which != 1) return fail(h, VQE_EINVAL, "vqe_lanczos: which must be 0 (lowest) or 1 (highest)");
  if (d.max_basis < 2) return fail(h, VQE_EINVAL, "vqe_lanczos: max_basis must be at least 2");
  if (d.max_matvec < 1) return fail(h, VQE_EINVAL, "vqe_lanczos: max_matvec must be at least 1");
  if (d.check_every < 1) return fail(h, VQE_EINVAL, "vqe_lanczos: check_every must be at least 1");
  if (!(d.tol > 0.0) || !std::isfinite(d.tol)) return fail(h, VQE_EINVAL, "vqe_lanczos: tol must be positive and finite");
  *o = LzOptions{d.which, d.max_basis, d.max_matvec, d.check_every, d.start_from_init != 0, d.tol, d.seed};
  return VQE_OK;
}

int lanczos(vqe_t* h, const vqe_lanczos_opts_t* opts, double* eigenvalue, void* amps, bool amps_on_device, double info[4]) {
  if (!h) return VQE_EINVAL;
  if (!eigenvalue || !info) return fail(h, VQE_EINVAL, "bad arguments");
  LzOptions o;
  VQE_TRY(lanczos_check(h, opts, &o));
  HIP_TRY(h, hipSetDevice(h->dev));
  VQE_TRY(lz_upload_ham(h->lz, h->ham_host, h->ham_ver, h->stream, h->err));
  size_t free_b = 0, total_b = 0;
  HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
  h->last_run_dm = false;
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  const int rc = lz_run(h->lz, h->n, h->stream, (const double2*)h->init.p, o, free_b, eigenvalue, info, h->err);
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  VQE_TRY(rc);
  if (amps) {
    HIP_TRY(h, hipMemcpyAsync(amps, lz_vector(h->lz, h->n), ((size_t)16) << h->n,
                              amps_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (!amps_on_device) HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  return VQE_OK;
}

// Everything a vqe_lanczos_multi call can be refused for, before anything is launched or given up.
int lanczos_multi_check(vqe_t* h, const vqe_lanczos_multi_opts_t* opts, LzMultiOptions* o) {
  vqe_lanczos_multi_opts_t d;
  vqe_lanczos_multi_default_opts(&d);
  if (opts) d = *opts;
  if (!h->ham_set) return fail(h, VQE_ESTATE, "no Hamiltonian set");
  if (h->shard_world > 1)
    return fail(h, VQE_ESTATE, "vqe_lanczos_multi on a term-sharded handle: a shard's spectrum is not the Hamiltonian's");
  if (h->amp_world > 1)
    return fail(h, VQE_ESTATE, "vqe_lanczos_multi on an amplitude-sharded handle: it holds a slice of the register");
  if (d.which != 0 && d.which != 1) return fail(h, VQE_EINVAL, "vqe_lanczos_multi: which must be 0 (lowest) or 1 (highest)");
  const int64_t most = std::min<int64_t>((int64_t)1 << h->n, kLzMaxEig);
  if (d.n_eig < 1 || d.n_eig > most) return fail(h, VQE_EINVAL, "vqe_lanczos_multi: n_eig must be in 1 .. min(2^n, 64)");
  if (d.max_basis < 2) return fail(h, VQE_EINVAL, "vqe_lanczos_multi: max_basis must be at least 2");
  if (d.max_matvec < 1) return fail(h, VQE_EINVAL, "vqe_lanczos_multi: max_matvec must be at least 1");
  if (d.check_every < 1) return fail(h, VQE_EINVAL, "vqe_lanczos_multi: check_every must be at least 1");
  if (d.keep < 0 || d.keep >= d.max_basis - 1)
    return fail(h, VQE_EINVAL, "vqe_lanczos_multi: keep must be 0 (the library's rule) or in 1 .. max_basis - 2");
  if (!(d.tol > 0.0) || !std::isfinite(d.tol)) return fail(h, VQE_EINVAL, "vqe_lanczos_multi: tol must be positive and finite");
  *o = LzMultiOptions{d.which, d.n_eig, d.max_basis, d.max_matvec, d.check_every, d.keep, d.tol, d.seed};
  return VQE_OK;
}

int lanczos_multi(vqe_t* h, const vqe_lanczos_multi_opts_t* opts, double* eigenvalues, void* amps, bool amps_on_device,
                  double* residuals, double info[5]) {
  if (!h) return VQE_EINVAL;
  if (!eigenvalues || !residuals || !info) return fail(h, VQE_EINVAL, "bad arguments");
  LzMultiOptions o;
  VQE_TRY(lanczos_multi_check(h, opts, &o));
  HIP_TRY(h, hipSetDevice(h->dev));
  VQE_TRY(lz_upload_ham(h->lz, h->ham_host, h->ham_ver, h->stream, h->err));
  size_t free_b = 0, total_b = 0;
  HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
  h->last_run_dm = false;
  int order[kLzMaxEig];
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  const int rc = lz_run_multi(h->lz, h->n, h->stream, o, free_b, eigenvalues, residuals, order, info, h->err);
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  VQE_TRY(rc);
  if (amps) {
    const size_t bytes = ((size_t)16) << h->n;
    for (int i = 0; i < (int)info[4]; ++i)
      HIP_TRY(h, hipMemcpyAsync((char*)amps + (size_t)i * bytes, lz_multi_vector(h->lz, h->n, order[i]), bytes,
                                amps_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (!amps_on_device) HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  return VQE_OK;
}
}  // namespace
}

int vqe_lanczos_multi_default_opts(vqe_lanczos_multi_opts_t* o) {
  if (!o) return VQE_EINVAL;
  *o = vqe_lanczos_multi_opts_t{0, 1, 128, 2000, 8, 0, 1e-10, 1ull};
  return VQE_OK;
}

int vqe_lanczos_multi(vqe_t* h, const vqe_lanczos_multi_opts_t* opts, double* eigenvalues, double* amps_re_im, double* residuals,
                      double info[5]) {
  return lanczos_multi(h, opts, eigenvalues, amps_re_im, false, residuals, info);
}

int vqe_lanczos_multi_dev(vqe_t* h, const vqe_lanczos_multi_opts_t* opts, double* eigenvalues, void* dev_amps_re_im,
                          double* residuals, double info[5]) {
  return lanczos_multi(h, opts, eigenvalues, dev_amps_re_im, true, residuals, info);
}

int vqe_lanczos_default_opts(vqe_lanczos_opts_t* o) {
  if (!o) return VQE_EINVAL;
  *o = vqe_lanczos_opts_t{0, 128, 2000, 8, 0, 1e-10, 1ull};
  return VQE_OK;
}

int vqe_lanczos(vqe_t* h, const vqe_lanczos_opts_t* opts, double* eigenvalue, double* amps_re_im, double info[4]) {
  return lanczos(h, opts, eigenvalue, amps_re_im, false, info);
}

int vqe_lanczos_dev(vqe_t* h, const vqe_lanczos_opts_t* opts, double* eigenvalue, void* dev_amps_re_im, double info[4]) {
  return lanczos(h, opts, eigenvalue, dev_amps_re_im, true, info);
}

int vqe_batch_energy_devptr(vqe_t* h, void** p) {
  if (!h || !p) return VQE_EINVAL;
  if (h->batch <= 0) return fail(h, VQE_ESTATE, "no batch loaded");
  *p = h->d_f.p;
  return VQE_OK;
}

int vqe_batch_copy_energy(vqe_t* h, void* dst_dev) {
  if (!h || !dst_dev) return VQE_EINVAL;
  if (h->batch <= 0) return fail(h, VQE_ESTATE, "no batch loaded");
  HIP_TRY(h, hipSetDevice(h->dev));
  HIP_TRY(h, hipMemcpyAsync(dst_dev, h->d_f.p, (size_t)h->batch * 8, hipMemcpyDeviceToDevice, h->stream));
  return VQE_OK;
}

int vqe_batch_set_trace(vqe_t* h, int enable) {
  if (!h) return VQE_EINVAL;
  if (enable && !h->lds_path) return fail(h, VQE_ESTATE, "evaluation traces are recorded by the fused device loop (n <= 13) only");
  h->trace_on = enable != 0;
  return VQE_OK;
}

int vqe_batch_fetch_trace(vqe_t* h, int circuit, double* out, int32_t* maxfun, int32_t* stride) {
  if (!h || !maxfun || !stride) return VQE_EINVAL;
  if (h->trace_maxfun <= 0) return fail(h, VQE_ESTATE, "no trace recorded: vqe_batch_set_trace(1), then a minimize / env-step run");
  if (circuit < 0 || circuit >= h->trace_batch) return fail(h, VQE_EINVAL, "circuit index out of range");
  *maxfun = h->trace_maxfun;
  *stride = h->trace_stride;
  if (!out) return VQE_OK;      // size query
  HIP_TRY(h, hipSetDevice(h->dev));
  const size_t words = (size_t)h->trace_maxfun * (size_t)h->trace_stride;
  HIP_TRY(h, hipMemcpyAsync(out, h->d_trace.p + (size_t)circuit * words, words * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return VQE_OK;
}

int vqe_debug_counters(vqe_t* h, uint64_t out[8]) {
  if (!h || !out) return VQE_EINVAL;
  HIP_TRY(h, hipSetDevice(h->dev));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(out, h->d_dbg.p, 64, hipMemcpyDeviceToHost));
#ifdef VQE_STAMPS   // slots 8..15: device-side COBYLA sections
  {
    static unsigned long long zero[8] = {0};
    HIP_TRY(h, hipMemcpyFromSymbol(cby_out_, HIP_SYMBOL(g_cby_dbg), 64));
    HIP_TRY(h, hipMemcpyToSymbol(HIP_SYMBOL(g_cby_dbg), zero, 64));
    std::fprintf(stderr, "cobyla sections:");
    for (int i = 0; i < 8; ++i) std::fprintf(stderr, " %llu", cby_out_[i]);
    unsigned long long io[2];
    HIP_TRY(h, hipMemcpyFromSymbol(io, HIP_SYMBOL(g_cby_in_out), 16));
    HIP_TRY(h, hipMemcpyToSymbol(HIP_SYMBOL(g_cby_in_out), zero, 16));
    std::fprintf(stderr, " | in %llu out %llu\n", io[0], io[1]);
  }
#endif
  HIP_TRY(h, hipMemset(h->d_dbg.p, 0, 64));
  return VQE_OK;
}

int vqe_last_kernel_ms(vqe_t* h, float* ms) {
  if (!h || !ms) return VQE_EINVAL;
  if (h->last_run_dm) { *ms = h->dm_gpu_ms; return VQE_OK; }      // exact channel mode: device time only (the host builds the blocks in between)
  HIP_TRY(h, hipEventSynchronize(h->ev1));
  HIP_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
  return VQE_OK;
}

int vqe_term_owner(int n_qubits, int n_terms, const uint64_t* xmask, int world, int32_t* owner) {
  if (n_qubits < 1 || n_qubits > 30 || n_terms < 0 || world < 1 || (n_terms > 0 && (!xmask || !owner))) return VQE_EINVAL;
  std::map<uint32_t, int> index;
  std::vector<uint32_t> gx;
  std::vector<std::vector<int>> terms;
  for (int k = 0; k < n_terms; ++k) {
    const uint32_t x = (uint32_t)xmask[k];
    auto it = index.find(x);
    if (it == index.end()) { it = index.emplace(x, (int)gx.size()).first; gx.push_back(x); terms.emplace_back(); }
    terms[it->second].push_back(k);
  }
  const std::vector<int> go = assign_groups(gx, terms, n_qubits <= 13, world);
  for (size_t g = 0; g < gx.size(); ++g) for (int k : terms[g]) owner[k] = go[g];
  return VQE_OK;
}

// ---- host COBYLA ---------------------------------------------------------------------------
struct vqe_cobyla {
  cby::CobylaM0<cby::HostCtx, true> c;
  std::vector<double> mem;
  int n = 0, want = 0, nfev = 0;
  double flast = 0.0;
  bool finished = false;
};

int vqe_cobyla_create(int n, const double* x0, double rhobeg, double rhoend, int maxfun, vqe_cobyla_t** out) {
  if (!out || n < 0 || (n > 0 && !x0) || maxfun < 1 || !(rhobeg > 0) || !(rhoend > 0)) return VQE_EINVAL;
  vqe_cobyla* c = new (std::nothrow) vqe_cobyla;
  if (!c) return VQE_ENOMEM;
  c->n = n;
  c->mem.assign(cby::scratch_doubles(n, 1) + 8, 0.0);
  c->c.bind(c->mem.data(), n);
  for (int i = 0; i < n; ++i) c->c.x[i] = x0[i];
  if (n == 0) { c->want = 1; c->c.nfvals = 1; c->c.status = cby::RUNNING; }
  else c->want = c->c.start(rhobeg, rhoend, maxfun);
  *out = c;
  return VQE_OK;
}

int vqe_cobyla_ask(vqe_cobyla_t* c, double* x) {
  if (!c) return VQE_EINVAL;
  if (!c->want) return 0;
  if (x) for (int i = 0; i < c->n; ++i) x[i] = c->c.x[i];
  return 1;
}

int vqe_cobyla_tell(vqe_cobyla_t* c, double f) {
  if (!c || !c->want) return VQE_ESTATE;
  c->flast = f;
  if (c->n == 0) { c->want = 0; c->c.status = cby::DONE_RHOEND; c->c.ifull = 1; return 0; }
  c->want = c->c.tell(f);
  return c->want;
}

int vqe_cobyla_result(vqe_cobyla_t* c, double* x, double* f, int32_t* nfev, int32_t* status) {
  if (!c) return VQE_EINVAL;
  if (x) for (int i = 0; i < c->n; ++i) x[i] = c->c.x[i];
  if (f) *f = (c->c.status == cby::DONE_RHOEND && c->c.ifull == 1) ? c->flast : c->c.fbest_ret;
  if (nfev) *nfev = c->c.nfvals;
  if (status) *status = c->c.status;
  return VQE_OK;
}

void vqe_cobyla_destroy(vqe_cobyla_t* c) { delete c; }

}  // extern "C"
