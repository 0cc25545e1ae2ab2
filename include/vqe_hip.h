/* vqe_hip.h - C ABI of the MI355X VQE environment-step engine (libvqe_hip.so).
 *
 * The reference (Aqasch/TensorRL-QAS) has no FFI: its hot path is Python calling the
 * third-party qulacs / numpy / scipy packages.  Each entry point below names the reference
 * interface it replaces (paths relative to the reference checkout).  Plain C types only;
 * every function returns 0 on success or a negative VQE_E* code and never throws or
 * aborts across the ABI; vqe_last_error() returns the message of the last failure.
 *
 * Conventions (identical to the reference's simulator, qulacs):
 *   - qubit k is bit k of the basis-state index (little-endian);
 *   - amplitudes are complex128, interleaved (re, im);
 *   - rotations are exp(+i*theta/2*P)  (qulacs add_parametric_R{X,Y,Z}_gate);
 *   - Pauli terms are (xmask, zmask, coeff): bit k of xmask set iff the factor on qubit k
 *     is X or Y, bit k of zmask set iff it is Z or Y; the i^{#Y} phase is applied by the
 *     callee.
 * A handle is not thread-safe; distinct handles are independent.  All work of a handle is
 * issued on one HIP stream (vqe_set_stream); calls that return results in host memory
 * block until those results are ready.
 */
#ifndef VQE_HIP_H
#define VQE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vqe_handle vqe_t;
typedef struct vqe_cobyla vqe_cobyla_t;

enum {
  VQE_OK = 0,
  VQE_EINVAL = -22,   /* bad argument */
  VQE_ENOMEM = -12,   /* host or device allocation failed */
  VQE_ENODEV = -19,   /* no usable HIP device */
  VQE_EHIP = -5,      /* a HIP runtime call failed */
  VQE_ESTATE = -1     /* call sequence error (e.g. no circuit / Hamiltonian set) */
};

/* gate kinds of a circuit description (order = reference construct_ansatz order,
 * environments/VQAs/VQE_qulacs_TN_notin_RL.py:13-45; noise kinds:
 * VQE_qulacs_TN_notin_RL_noise.py:26-28,40-50; two-qubit Pauli rotations of the SU(4) gate set:
 * environments/VQAs/VQE_qulacs_su4.py:68-90, ParametricPauliRotation([q0, q1], [P, P], theta)) */
enum {
  VQE_GATE_CNOT = 0,   /* q0 = control, q1 = target                       */
  VQE_GATE_RX = 1,     /* q0 = qubit, param_idx = index into theta        */
  VQE_GATE_RY = 2,
  VQE_GATE_RZ = 3,
  VQE_GATE_DEPOL1 = 4, /* DepolarizingNoise(q0, p1)                       */
  VQE_GATE_DEPOL2 = 5, /* TwoQubitDepolarizingNoise(q0, q1, p2)           */
  VQE_GATE_RXX = 6,    /* exp(+i*theta/2 * X_q0 X_q1), q0 != q1, param_idx */
  VQE_GATE_RYY = 7,    /* exp(+i*theta/2 * Y_q0 Y_q1)   (symmetric in q0, q1; the exact channel   */
  VQE_GATE_RZZ = 8     /* exp(+i*theta/2 * Z_q0 Z_q1)    mode takes them after vqe_set_dm_rot2)   */
};

/* ---- lifetime ------------------------------------------------------------------------
 * replaces: qulacs.QuantumState(n) / ParametricQuantumCircuit(n) construction,
 * environments/VQAs/VQE_qulacs_TN_notin_RL.py:10,82 */
int vqe_create(int n_qubits, int device_id, vqe_t** out);
void vqe_destroy(vqe_t* h);
const char* vqe_last_error(const vqe_t* h); /* h may be NULL: last error of vqe_create */
int vqe_set_stream(vqe_t* h, void* hip_stream); /* NULL: the handle's own stream */
/* the stream all work of the handle is issued on (its own one unless vqe_set_stream replaced it):
 * lets the caller order its own streams against it (e.g. torch.cuda.ExternalStream + wait_stream
 * before an RCCL all-reduce of vqe_batch_copy_energy's destination) */
int vqe_get_stream(vqe_t* h, void** hip_stream);
int vqe_sync(vqe_t* h);
/* device facts for the caller's roofline arithmetic: [0]=CU count, [1]=LDS bytes/CU,
 * [2]=workgroups resident per CU for the last LDS-path launch, [3]=1 if the LDS-resident
 * path serves this n_qubits else 0 */
int vqe_device_info(vqe_t* h, int64_t info[4]);

/* ---- problem definition --------------------------------------------------------------
 * replaces: state.load(TN_state)            VQE_qulacs_TN_notin_RL.py:83
 *           (NULL = |0...0>, the VQE_qulacs.py:81 path) */
int vqe_set_init_state(vqe_t* h, const double* amps_re_im /* 2 * 2^n, or NULL */);
/* The same with the amplitudes in DEVICE memory (complex128, 2^n, e.g. a torch tensor): an asynchronous
 * device-to-device copy on the handle's stream.  vqe_get_state_dev is vqe_get_state with a device destination.
 * Used by the amplitude-sharded states (tensorrl-qas_amd/parallel.py), where a rank's shard of a larger register is
 * the "state" of an (n - log2 world)-qubit handle and never leaves the GPU between two exchanges. */
int vqe_set_init_state_dev(vqe_t* h, const void* dev_amps_re_im);
int vqe_get_state_dev(vqe_t* h, const double* theta, void* dev_amps_re_im);
/* replaces: the dense operator handed to get_exp_val (VQE_qulacs_TN_notin_RL.py:80,86;
 * built at environment_qulacs_TN_notin_agent.py:126-131,162) by its Pauli-sum form */
int vqe_set_hamiltonian_pauli(vqe_t* h, int n_terms, const uint64_t* xmask,
                              const uint64_t* zmask, const double* coeff);
/* The same operator as the reference hands it to get_exp_val: a dense 2^n x 2^n complex matrix in the
 * simulator's little-endian basis, row-major, (re, im) interleaved - i.e. the product of
 * Operator(H).reverse_qargs().to_matrix() (environment_qulacs_TN_notin_agent.py:162) on the fixed path, the raw
 * file matrix on the trainable path.  Decomposed into Pauli terms on the host (one Walsh-Hadamard transform
 * per X mask; coefficients below tol * max|H_ij| are dropped; n <= 13).  vqe_hamiltonian_terms reports what
 * was found. */
int vqe_set_hamiltonian_dense(vqe_t* h, const double* op_re_im /* 2 * 4^n */, double tol);
int vqe_hamiltonian_terms(vqe_t* h, int32_t* n_terms, int32_t* n_xgroups);
/* How the LDS-resident kernels hold this handle's share of the Hamiltonian (diagnostic; n <= 13):
 * out[0] = X-mask groups evaluated through full sign-sum tables, out[1] = units - sub-cubes of
 * one pair per thread on which the table of a mostly-zero group (a fermionic excitation operator
 * connects one occupation pattern in 2^w) does not vanish; groups stored as units are not in
 * out[0] -, out[2] = groups of out[0] whose partner index sits in the register bits, out[3] = 1
 * if there is a diagonal group.  The reference has no counterpart: its get_exp_val multiplies
 * by the dense matrix (VQE_qulacs_TN_notin_RL.py:86). */
int vqe_hamiltonian_layout(vqe_t* h, int32_t out[4]);
/* Where the device COBYLA of the LDS-resident kernels (n <= 13) keeps its arrays for ONE circuit, and which of its
 * update contexts runs (diagnostic, for tests that must know which code path a circuit took; the answer comes from
 * the function the kernel itself calls).  It depends on the sizes of the whole resident batch - max_ops (rotations and
 * noise ops of the longest circuit), max_pair (its RX / RY / RXX / RYY gates), max_params, each as the library rounds
 * them up to a multiple of 4 -, on the X-mask groups of the Hamiltonian, on whether the launch is the variant for
 * batches with a circuit of more than 64 parameters (wide), and on the circuit's own parameter count n_params:
 *   out[0] class: VQE_COBYLA_RESIDENT an LDS region of their own (n <= 9 and the workgroup still fits eight times into
 *          a CU); _STAGED copied into the idle state region of LDS around every update; _GLOBAL in the global scratch,
 *          one wavefront, one lane per row; _ROWS the same with row walks through an LDS tile (wide launches at n <= 9,
 *          more than 32 parameters); _BLOCK in the global scratch, updated by the whole workgroup (wide launches at
 *          n >= 10, more than 64 parameters)
 *   out[1] padding of the inner loops (8 or 16), out[2] doubles the arrays take in that layout,
 *   out[3] dynamic LDS bytes of the launch, out[4] 1 if two lanes share a row (at most 32 parameters, one-wave contexts),
 *   out[5] bytes of the LDS tile of the one-wave wide launch (0 in every other launch), out[6] bytes of the LDS region of class
 *   RESIDENT (else 0), out[7] 1 if the launch is accepted (LDS within 160 KiB - the handle variant: within the
 *   device's figure -, at most 2^n ops from n = 10).
 * vqe_cobyla_placement is host only (needs no device) and takes the sizes as given (VQE_EINVAL for wide != 0 below
 * 6 qubits or with max_params <= 64: no launch runs that variant there); vqe_batch_cobyla_placement answers
 * for circuit `circuit` of the resident batch with the handle's own sizes, for a plain vqe_batch_run_minimize (an
 * environment step whose new gate is a rotation optimises one variable less).  The reference has no counterpart. */
enum { VQE_COBYLA_RESIDENT = 0, VQE_COBYLA_STAGED = 1, VQE_COBYLA_GLOBAL = 2, VQE_COBYLA_ROWS = 3, VQE_COBYLA_BLOCK = 4 };
int vqe_cobyla_placement(int n_qubits, int max_ops, int max_pair, int max_params, int n_groups, int n_params, int wide,
                         int64_t out[8]);
int vqe_batch_cobyla_placement(vqe_t* h, int circuit, int64_t out[8]);
/* LDS bank conflicts of the unit path's ds_read_b128 (model: four groups of 16 lanes per wave): out = {mean, worst}
 * number of a group's lanes that share one 16-byte slot with the plain state layout, then {mean, worst} with the bank
 * swizzle the handle chose (1 = conflict free; the identity where no swizzle applies). */
int vqe_unit_bank_score(vqe_t* h, double out[4]);
/* Evaluate only the X-mask groups owned by `rank` of `world` (Pauli-term sharding; the
 * caller sums the partial energies of all ranks, e.g. one RCCL all-reduce). */
int vqe_set_term_shard(vqe_t* h, int rank, int world);
/* Streaming path (n >= 14) only: sweep slice `rank` of `world` equal slices of the amplitude
 * index range for ALL terms (the other partition of the double sum over terms and basis
 * states).  Every rank still applies the whole circuit to its own copy of the state; the
 * partial energies are summed by the caller exactly as for term sharding.  Work and memory
 * traffic of the reduction are 1/world per rank. */
int vqe_set_amplitude_shard(vqe_t* h, int rank, int world);
/* n >= 14: allow vqe_energy_grad_batch / vqe_batch_run_energy_grad on the streaming path (a second
 * state-sized buffer per resident stream).  0 (default): VQE_EINVAL as before.  n <= 13: accepted, no effect. */
int vqe_set_stream_grad(vqe_t* h, int enable);
/* n >= 14: allow vqe_minimize_lbfgs / vqe_batch_run_minimize_lbfgs / vqe_batch_run_env_step_lbfgs on the streaming
 * path (a second state-sized buffer per resident stream, as vqe_set_stream_grad).  0 (default): VQE_EINVAL as before,
 * whatever vqe_set_stream_grad says.  n <= 13: accepted, no effect.  Independent of vqe_set_stream_grad. */
int vqe_set_stream_lbfgs(vqe_t* h, int enable);
/* Paired env-step launches (10 <= n <= 13).  1 (default): vqe_batch_run_minimize / vqe_batch_run_env_step put two
 * environments of the batch into one workgroup (neighbours in the launch order) where the launch is the plain
 * noiseless minimiser - no depolarising or shot noise, at most 64 parameters per circuit, no evaluation trace -, the
 * batch has at least five parameters per circuit on average (below, pairing measured slower) and the larger LDS
 * footprint leaves the workgroups per CU unchanged: both are evaluated in turn, then their two COBYLA
 * updates run at the same time on two wavefronts.  Every environment's result is, bit for bit, that of the unpaired
 * launch.  0: every launch is unpaired.  Other sizes and runs: accepted, no effect. */
int vqe_set_env_pairing(vqe_t* h, int enable);
/* What the last launch of an LDS-resident kernel (n <= 13) on this handle did: out[0] = 1 if it was the paired
 * kernel, out[1] = workgroups with two environments, out[2] = workgroups of the paired kernel with one environment
 * (the tail of the launch order), out[3] = dynamic LDS bytes per workgroup.  An unpaired launch: 0, 0, 0, bytes. */
int vqe_last_env_pairing(vqe_t* h, int64_t out[4]);
/* Host only: the LDS layout of a paired launch with these batch sizes (10 <= n_qubits <= 13).  out[0..7]: byte offsets
 * of the second environment's sched, lay, cs, xm, zm, meta, sb, sidx regions; out[8]: offset of the two 64-byte
 * environment records; out[9]: dynamic LDS bytes of the paired launch; out[10]: those of the unpaired launch (the
 * first environment's regions and the shared ones lie below it); out[11]: bytes of the state region, which starts at
 * offset 0. */
int vqe_pair_lds_plan(int n_qubits, int max_ops, int max_pair, int max_params, int n_groups, int64_t out[12]);
/* The one collective of the term-sharded sum as a library call (RCCL over xGMI; librccl is opened lazily).  Rank 0
 * makes the 128-byte id (vqe_comm_unique_id) and hands it to the other ranks by any means; every rank calls
 * vqe_comm_init on its handle; vqe_comm_allreduce_energy sums the batch's energy array (float64[batch], what
 * vqe_batch_run_energy left on the device and vqe_batch_fetch returns) over the ranks, in place, asynchronously on
 * the handle's stream.  The reference has no counterpart (single process). */
int vqe_comm_unique_id(void* id128);
int vqe_comm_init(vqe_t* h, int rank, int world, const void* id128);
int vqe_comm_allreduce_energy(vqe_t* h);
int vqe_comm_destroy(vqe_t* h);
/* host only: the rank that vqe_set_term_shard(.., world) makes responsible for each term
 * (terms sharing an X mask stay together); needs no device */
int vqe_term_owner(int n_qubits, int n_terms, const uint64_t* xmask, int world, int32_t* owner);
/* Stochastic Pauli noise (qulacs DepolarizingNoise / TwoQubitDepolarizingNoise
 * semantics: each non-identity Pauli with probability p/3 resp. p/15, one trajectory per
 * evaluation).  The draw for (stream, evaluation, gate) is a pure function of `seed`; stream = position of the
 * circuit in the resident batch, evaluation = the handle's evaluation counter:
 *   - vqe_create and every vqe_set_noise set the counter to 0 (nothing else does: not vqe_set_shot_noise, not a new
 *     Hamiltonian, circuit, batch or initial state);
 *   - an energy run (vqe_energy*, vqe_batch_run_energy) or a state (vqe_get_state*) draws at the counter, then adds 1;
 *   - a gradient-free optimiser run (vqe_minimize_cobyla, vqe_batch_run_minimize, vqe_batch_run_env_step) with `maxfun`
 *     draws its k-th evaluation at counter + k (k = 1 .. nfev), an env-step's final evaluation of the full circuit at
 *     counter + maxfun + 1, then adds maxfun + 1 - whatever nfev was;
 *   - exact-channel runs (the energies and optimiser runs of vqe_set_noise_mode 1), gradient and device L-BFGS runs,
 *     vqe_batch_run_reduction and every refused call leave it unchanged.  vqe_get_state* has no exact-channel form: in
 *     mode 1 too it is a trajectory at the counter and adds 1.  The counter counts with noise off as well.
 * One seed per handle: vqe_set_noise and vqe_set_shot_noise both set it, for the Pauli draws and the shot draws alike,
 * and the later call wins.  VQE_EINVAL (handle unchanged) for a probability outside [0, 1]. */
int vqe_set_noise(vqe_t* h, double p1, double p2, uint64_t seed);
/* How the noise gates of a circuit are evaluated.  0 (default): one Pauli trajectory per evaluation, as qulacs does
 * inside update_quantum_state (VQE_qulacs_TN_notin_RL_noise.py:94-101).  1: the exact channel those draws sample
 * from - density-matrix evolution rho -> (1-p) rho + p/3 sum_P P rho P (two qubits: p/15 over the 15 non-identity
 * Paulis), E = tr(rho H); 2 <= n <= 13 (4^n complex128 in HBM), runs of gates inside a two-qubit window fused into
 * 16 x 16 superoperators applied with FP64 MFMA; vqe_energy*, vqe_batch_run_energy, vqe_minimize_cobyla,
 * vqe_batch_run_minimize / _env_step.  By default COBYLA is driven by the host on the exact energies, one circuit and
 * one evaluation at a time; after vqe_set_dm_batched the resident batch is evaluated in lock-step and COBYLA runs on
 * the device.  The seed of vqe_set_noise and vqe_set_shot_noise play no part in mode 1. */
int vqe_set_noise_mode(vqe_t* h, int mode);
/* Exact channel mode only: evaluate the resident batch in lock-step on the device.
 * max_resident  0 (default): the serial host-driven path, as before.
 *              -1: as many density matrices resident as fit into a quarter of the free device
 *                  memory at the first batched run (at least 1, at most the batch);
 *             R>=1: at most R.
 * Accepted in any noise mode and for any n; it takes effect when mode 1 runs (2 <= n <= 13 as before).  The block
 * structure of every circuit is planned once per resident batch, the 16 x 16 matrices are rebuilt on the device for
 * every trial point, all circuits of a chunk of R sweep side by side and COBYLA of vqe_minimize_cobyla /
 * vqe_batch_run_minimize / _env_step runs on the device (one thread per circuit, the host build's arithmetic).  The
 * energy of a circuit has the same bits whatever the batch around it, its position and R; the bits of the serial path
 * are not promised (the device-built matrices may differ from the host-built ones in the last place). */
int vqe_set_dm_batched(vqe_t* h, int max_resident);
/* out[0] density matrices resident per chunk in the last batched run, [1] chunks per lock-step
 * evaluation, [2] lock-step evaluations of the last run that evaluated at least one circuit (1 for an energy run; the
 * largest nfev of a minimisation, one more for an env-step), [3] block levels (sweeps per chunk and evaluation: the
 * largest block count of a resident circuit).  All 0 after a serial run. */
int vqe_dm_batch_info(vqe_t* h, int64_t out[4]);
/* Exact channel mode on the batched path only: serve vqe_energy_grad_batch, vqe_batch_run_energy_grad /
 * vqe_batch_fetch_grad and the device L-BFGS (vqe_minimize_lbfgs, vqe_batch_run_minimize_lbfgs / _env_step_lbfgs) by the
 * adjoint gradient of tr(rho H): forward sweeps with rho_0 .. rho_L kept, Lambda = conj(H) swept back with the adjoint
 * blocks, one 16 x 16 matrix per block contracted with the block's derivative.  0 (default): those calls are refused in
 * mode 1 as before.  Accepted on any handle; it takes effect in mode 1 with vqe_set_dm_batched != 0 (with the serial
 * path those calls stay refused, VQE_ESTATE).  A resident circuit costs levels + 2 density matrices, so out of the same
 * budget (max_resident density matrices, or a quarter of the free memory) fewer circuits are resident than in an
 * energy run - vqe_dm_batch_info reports the count - and VQE_ENOMEM when not even one fits.  The gradient of a circuit
 * has the same bits whatever the batch around it, its position and max_resident.  Noise counter: unchanged. */
int vqe_set_dm_grad(vqe_t* h, int enable);
/* Exact channel mode only: Kraus sets in the two noise slots (csrc/dm_host.h).  The channel applied at
 * VQE_GATE_DEPOL1 gates becomes rho -> sum_k K1_k rho K1_k^+ (K1: n1 x 2 x 2 complex, re / im interleaved, row-major), the
 * one at VQE_GATE_DEPOL2 gates sum_k K2_k rho K2_k^+ (K2: n2 x 4 x 4, basis index = bit(q0) + 2 bit(q1) of the GATE's two
 * qubits in the gate's order - a channel need not be symmetric in them).  n1 == 0 leaves that slot on the depolarising
 * channel of vqe_set_noise (p1), n2 == 0 likewise (p2); both 0 removes the override.  0 <= n1 <= 16, 0 <= n2 <= 64.
 * VQE_EINVAL with the handle unchanged for a count out of range, a NULL array with a positive count, or a set that is
 * not trace preserving (max |sum K^+ K - I| > 1e-12).  The call touches neither the seed, the noise counter, p1 / p2 nor
 * the results of the resident batch; a later vqe_set_noise does not remove the override.
 * While an override is installed the mode 1 runs use it - energies, COBYLA and env-steps on the serial and the batched
 * path, gradient and L-BFGS under vqe_set_dm_grad - and what has no form for a general channel is refused with
 * VQE_ESTATE before anything is loaded or launched, noise counter unchanged: every energy, gradient, state, reduction
 * and optimiser run of mode 0, and vqe_get_state* in any mode.  Without an override nothing changes. */
int vqe_set_noise_kraus(vqe_t* h, int n1, const double* K1, int n2, const double* K2);
/* out[0], out[1]: Kraus operators installed in the one- / two-qubit slot, 0 = none */
int vqe_noise_kraus_info(vqe_t* h, int32_t out[2]);
/* Pauli channels in the two noise slots (csrc/noise_pauli.h): qulacs BitFlipNoise, DephasingNoise,
 * IndependentXZNoise, or any biased channel rho -> w_0 rho + sum_k w_k P_k rho P_k.  w1[k - 1], k = 1 .. 3: the
 * probability of X, Y, Z at a VQE_GATE_DEPOL1 gate.  w2[k - 1], k = 1 .. 15: the probability of code k = a | b << 2 at a
 * VQE_GATE_DEPOL2 gate, a acting on q0 and b on q1, each 1 = X, 2 = Y, 3 = Z.  The identity's probability w_0 is the
 * remainder.  NULL leaves that slot on the depolarising channel of p1 / p2; both NULL removes the tables.
 * The draw: cum_0 = 0, cum_k = cum_{k-1} + w_k in this order in double; u is the uniform of the depolarising draw - same
 * hash, key and position numbering in the executed (pre-action) gate list; the code is 0 where u >= cum_m, else the
 * smallest k with u < cum_k, so an entry with w_k = 0 is never selected.  A slot without a table keeps the rule
 * 1 + (int)(u / p * m) and its bits; a table with w_k = p / m is not promised to reproduce that rule at marginal draws.
 * A table is the generalisation of p1 / p2: wherever the depolarising channel of its slot is used, the table's channel
 * is used instead - the mode 0 sampler on the LDS-resident and the streaming path (energies, states, reduction, device
 * COBYLA, env-step), mode 1 (serial, batched, gradient and L-BFGS under vqe_set_dm_grad) and the quantum-jump runs of
 * vqe_set_kraus_traj for a slot without an override, through the Kraus set sqrt(w_0) 1, sqrt(w_k) P_k in the order
 * k = a + 4 b.  A Kraus override on a slot wins over the table, as it wins over p1 / p2.  Mode 0 gradients and L-BFGS
 * stay refused while a table has a positive total, as for depolarising noise, unless vqe_set_noise_grad switched the
 * gradients of frozen realisations on.  Term-sharded handles serve the tables.
 * The call touches neither the seed, the evaluation counter, p1 / p2, a Kraus override nor the results of the resident
 * batch; a later vqe_set_noise does not remove a table; the counter rules of vqe_set_noise hold unchanged.
 * VQE_EINVAL, handle unchanged, for a NaN, an entry outside [0, 1] or a total above 1 + 1e-12; VQE_ESTATE on an
 * amplitude-sharded handle (and vqe_set_amplitude_shard refuses a world > 1 while a table is installed). */
int vqe_set_noise_pauli(vqe_t* h, const double* w1 /* 3, or NULL */, const double* w2 /* 15, or NULL */);
/* out[0], out[1]: 1 where a table is installed in the one- / two-qubit slot, else 0 */
int vqe_noise_pauli_info(vqe_t* h, int32_t out[2]);
/* Mode 0 Pauli noise: adjoint gradient and device L-BFGS on frozen draws (csrc/vqe_grad.h).
 * n_real = T, 0 <= T <= 4096.  T = 0 is off, which is the default.  It is refused on an amplitude-sharded handle with
 * VQE_ESTATE.  That matches vqe_set_noise_pauli.
 * While on, with mode 0 and Pauli noise installed (depolarising p1 / p2 or a vqe_set_noise_pauli table), the gradient and
 * L-BFGS entry points are served at n <= 13 instead of refused (at 14 <= n <= 20 after vqe_set_stream_noise_grad, below).
 * The value they differentiate is
 *   E_T(theta) = (1/T) sum_{t=0}^{T-1} E(theta; draws of (seed, stream b, evaluation id eval_base + t)),
 * summed in ascending t.  The draws are exactly those that vqe_batch_run_energy uses for evaluation id eval_base + t of
 * batch position b.  Noise gates are numbered by position in the executed gate list.  The gradient is
 * (1/T) sum_t dE/dtheta in the same order.  The result has the same bits for the same (seed, eval_base, batch position, T).
 * The counter:
 *  - vqe_energy_grad_batch / vqe_batch_run_energy_grad: eval_base += T after the run.  With hold != 0 the counter stays,
 *    and vqe_noise_grad_advance adds T.  A host optimiser then sees one deterministic function per run.
 *  - vqe_minimize_lbfgs / vqe_batch_run_minimize_lbfgs: every evaluation of the run uses the same T realisations.
 *    Afterwards eval_base += T, whatever hold is.
 *  - vqe_batch_run_env_step_lbfgs: the optimisation runs on the pre-action circuit with the T realisations.  The one
 *    closing energy of the full circuit is a single trajectory with id eval_base + T (the COBYLA env-step also reports
 *    one draw there).  Afterwards eval_base += T + 1.
 * Still refused, with the codes they had: shot noise, Kraus sets without a Pauli form and vqe_set_kraus_traj runs (their
 * probabilities depend on theta), L-BFGS on a term shard.  A term-sharded handle gets its partial E_T and its
 * partial gradient, as without noise; every rank draws the same errors.  A refused call changes nothing.
 * With the switch off, every call answers as before.  With the switch on and p1 = p2 = 0 and no table, the noiseless
 * kernels run and their bits are unchanged.  VQE_EINVAL, handle unchanged, for T outside [0, 4096]. */
int vqe_set_noise_grad(vqe_t* h, int n_real, int hold);
/* eval_base += T (the T of vqe_set_noise_grad; nothing with the switch off) */
int vqe_noise_grad_advance(vqe_t* h);
/* out[0] T, [1] hold, [2] the current eval_base, [3] 0 */
int vqe_noise_grad_info(vqe_t* h, int64_t out[4]);
/* The same gradients on the streaming path (14 <= n <= 20, csrc/vqe_stream_grad.h), opt-in per handle.
 * max_resident: 0 (default) off - a handle with n >= 14 answers every call as before, code and text; -1 on, with as many
 * (circuit, realisation) states resident as fit into a quarter of the free device memory at the first run (at least 1,
 * at most batch x T); R >= 1 on, with at most R resident; < -1 VQE_EINVAL, handle unchanged.  VQE_ESTATE on an
 * amplitude-sharded handle.  Accepted with no effect at n <= 13.  Touches neither seed, counter, tables nor the resident
 * batch.  With the switch on, mode 0, Pauli noise installed and vqe_set_noise_grad(T >= 1), the entry points
 * vqe_set_noise_grad lists are served with its E_T, word for word, and its counter rules; the gradient calls need
 * vqe_set_stream_grad beside it, the L-BFGS calls vqe_set_stream_lbfgs, and without those their own refusals stay, in
 * the existing order.  The batch x T pairs run as streams of one set of launches, max_resident at a time; a pair holds
 * two states of 16 * 2^n bytes.  The results have the same bits for the same (seed, eval_base, batch position, T),
 * whatever max_resident and whatever else is in the batch.  The refusals of vqe_set_noise_grad stay. */
int vqe_set_stream_noise_grad(vqe_t* h, int max_resident);
/* out[0] max_resident as set, [1] pairs resident per chunk in the last served run, [2] chunks of that run (per
 * evaluation), [3] 0 */
int vqe_stream_noise_grad_info(vqe_t* h, int64_t out[4]);
/* Mode 0 under a Kraus override (vqe_set_noise_kraus): evaluate an energy as the mean of n_traj quantum-jump
 * trajectories.  0 (default): those runs are refused with VQE_ESTATE as before.  1 .. 4096.  Accepted on any handle;
 * takes effect in mode 0 while an override is installed, 1 <= n <= 13, unsharded handles.  Touches neither seed,
 * counter, p1/p2, the override nor the resident batch's results.  VQE_EINVAL, handle unchanged, for a count outside
 * [0, 4096].
 * A trajectory (csrc/vqe_qjump.h).  The draw of (stream b, evaluation e, trajectory t, noise gate at position g of the
 * executed gate list) is u = noise_uniform_k(noise_key(seed, b, e), ((uint64_t)(t + 1) << 44) | g), the hash of the Pauli
 * draws; g is numbered as there (gates left out by an env-step's pre-action rule do not count), one draw per noise
 * gate.  With rho_red the reduced density matrix of the gate's one or two qubits (index = bit(q0) + 2 bit(q1)) and
 * p_k = tr(K_k^+ K_k rho_red), k is the smallest index with u < p_0 + ... + p_k (accumulated in k order in double; if
 * rounding leaves none, the last k with p_k > 0), and psi <- K_k psi / sqrt(p_k).  A slot without an override (n1 == 0 or
 * n2 == 0) runs the depolarising Kraus set of its p1 / p2 - sqrt(1 - p) 1, then sqrt(p / 3) X, Y, Z resp.
 * sqrt(p / 15) P_b (x) P_a at k = a + 4 b - and is the identity, skipped, at probability 0.
 * The energy of an evaluation is the mean over t = 0 .. n_traj - 1 of <psi_t|H|psi_t>, summed in t order, plus
 * shot_sigma * noise_gauss(seed, b, e) once per evaluation.  The same seed, counter, batch position and n_traj give the
 * same bits, whatever the batch around the circuit.  The counter follows the mode 0 rules of vqe_set_noise: an energy
 * run or a state draws at the counter and adds 1, an optimiser run with maxfun draws its k-th evaluation at counter + k,
 * an env-step its final full-circuit evaluation at counter + maxfun + 1, either then adds maxfun + 1; a refused call
 * leaves it alone.
 * Served: vqe_energy, vqe_energy_batch, vqe_batch_run_energy, vqe_minimize_cobyla, vqe_batch_run_minimize,
 * vqe_batch_run_env_step (COBYLA on the device, all circuits in lock-step), and vqe_get_state / vqe_get_state_dev in
 * either noise mode: the normalised state of trajectory 0 at the counter.  Still refused with VQE_ESTATE before anything
 * is loaded or launched: gradient and L-BFGS calls, vqe_batch_run_reduction, term- or amplitude-sharded handles,
 * n >= 14 (unless vqe_set_stream_kraus_traj switched the streaming path's trajectories on). */
int vqe_set_kraus_traj(vqe_t* h, int n_traj);
/* out[0] n_traj, [1] workgroups of the last trajectory launch (n >= 14: of the last state sweep launched), [2] jumps
 * (selections k != 0) of the last evaluation, summed over circuits and trajectories, [3] lock-step evaluations of the
 * last run (1 for an energy run) */
int vqe_kraus_traj_info(vqe_t* h, int64_t out[4]);
/* Quantum-jump trajectories on the streaming path (n >= 14, csrc/vqe_stream_qjump.h), opt-in per handle.  max_resident:
 * 0 (default) off - a handle with n >= 14 refuses trajectory runs with VQE_ESTATE as before, code and text; -1 on, with
 * as many (circuit, trajectory) states resident as fit into a quarter of the free device memory at the first run (at
 * least 1, at most batch x n_traj); R >= 1 on, with at most R resident; < -1 VQE_EINVAL, handle unchanged.  Accepted on
 * any handle; no effect at n <= 13, where the LDS-resident path keeps serving.  With the switch on, an override (or
 * depolarising slots beside one), vqe_set_kraus_traj(T >= 1) and n >= 14, every call vqe_set_kraus_traj lists as served
 * runs T trajectories per circuit, each a state of 16 * 2^n bytes in device memory, batch x T of them chunk by chunk:
 * the same trajectory definition, draws and counter rules.  The per-trajectory energies, the mean and the state of
 * trajectory 0 have the same bits for the same seed, counter, batch position and T, whatever the batch around the
 * circuit and whatever max_resident.  Still refused with VQE_ESTATE before anything is loaded or launched: sharded
 * handles, gradient, L-BFGS and reduction-only calls. */
int vqe_set_stream_kraus_traj(vqe_t* h, int max_resident);
/* out[0] states resident per chunk in the last run on that path, [1] chunks per evaluation, [2] jump rounds (the most
 * noise records of a resident circuit), [3] state sweeps launched per chunk and evaluation before the energy (the
 * initial state, the rotation sweeps of every round, two per jump round); all 0 before such a run */
int vqe_stream_kraus_traj_info(vqe_t* h, int64_t out[4]);
/* per-trajectory energies e[b * n_traj + t] of the last energy run, or of the final full-circuit evaluation of the last
 * env-step; VQE_ESTATE after anything else (a new batch, any other run, a vqe_set_kraus_traj that changes n_traj) */
int vqe_batch_fetch_traj(vqe_t* h, double* e /* batch x n_traj */);
/* 1: the exact channel mode takes VQE_GATE_RXX / RYY / RZZ - a two-qubit rotation is a member of a superoperator block
 * like a CNOT - on the serial and the batched path, gradient and L-BFGS included.  0 (default): refused with VQE_EINVAL
 * as before.  Accepted on any handle; it takes effect in mode 1. */
int vqe_set_dm_rot2(vqe_t* h, int enable);
/* host only (needs no device): the superoperator blocks the exact channel mode would sweep for this circuit - windows[2k],
 * windows[2k+1] = the two qubits (a, b) of block k, S[k][2][16][16] = real and imaginary part of its 16 x 16 matrix, entry
 * index = ket_a + 2 ket_b + 4 bra_a + 8 bra_b.  windows == NULL or S == NULL: only the count.  For tests of the fusion. */
int vqe_dm_plan(int n_qubits, int n_gates, const int32_t* kind, const int32_t* q0, const int32_t* q1, const int32_t* param_idx,
                const double* theta, double p1, double p2, int cap_blocks, int32_t* n_blocks, int32_t* windows, double* S);
/* out[0] = the mode, out[1] = superoperator blocks (sweeps over rho) of the last exact-mode evaluation; for the
 * caller's roofline arithmetic (a sweep reads and writes 4^n complex128) */
int vqe_noise_mode_info(vqe_t* h, int32_t out[2]);
/* Finite-shot model of the reference's restricted variant
 * (environments/VQAs/VQE_qulacs_TN_notin_RL_noise_restricted.py:47-48,84-96): every evaluation
 * returns E + weights . N(0, sigma^2 I), sigma = n_shots^-1/2, i.e. E + sigma_total * N(0,1)
 * with sigma_total = sigma * |weights|_2 (the same distribution, one draw per evaluation from
 * the seeded counter-based generator).  0 switches it off.  The draw of (stream, evaluation) is numbered by the same
 * evaluation counter as the Pauli draws (see vqe_set_noise); this call does NOT restart it.  `seed` replaces the
 * handle's one seed - also for the Pauli draws of a vqe_set_noise made earlier, and also when sigma_total is 0 -, and
 * a later vqe_set_noise replaces it in turn: callers that want both noises pass the same seed to both (CircuitEnv
 * does), or call vqe_set_noise first and know that the second seed is the one in force. */
int vqe_set_shot_noise(vqe_t* h, double sigma_total, uint64_t seed);

/* ---- one circuit ---------------------------------------------------------------------
 * replaces: Parametric_Circuit.construct_ansatz product (the qulacs circuit handle),
 * VQE_qulacs_TN_notin_RL.py:13-45 */
int vqe_set_circuit(vqe_t* h, int n_gates, const int32_t* kind, const int32_t* q0,
                    const int32_t* q1, const int32_t* param_idx, int n_params);
/* replaces: get_energy_qulacs / get_exp_val, VQE_qulacs_TN_notin_RL.py:48-87 */
int vqe_energy(vqe_t* h, const double* theta, double* energy);
int vqe_energy_batch(vqe_t* h, int batch, const double* theta /* batch x n_params */,
                     double* energy /* batch */);
/* Energy and its gradient dE/dtheta of the circuit set by vqe_set_circuit at `batch` parameter vectors, by the
 * adjoint method (one forward sweep, lambda = H psi, one backward sweep; the cost does not grow with the number of
 * parameters).  grad[b * P + j] sums over every gate with parameter index j (0 for a parameter no gate uses).
 * replaces: the finite-difference gradient scipy.optimize.minimize builds for a gradient method when the reference
 * passes no `jac` (environment_qulacs_TN_notin_agent.py:452-482 with optim_alg = BFGS, L-BFGS-B, ...): P + 1
 * sequential get_exp_val calls per gradient.  1 <= n <= 13: the LDS-resident kernel.  n >= 14: VQE_EINVAL unless
 * vqe_set_stream_grad(h, 1) was called; then the streaming path computes it (forward sweeps, lambda = H psi in a second
 * state-sized buffer, backward sweeps over both).  Such a call undoes the circuit on the resident states: a
 * vqe_batch_run_reduction right after it is refused with VQE_ESTATE.  Refused with
 * VQE_ESTATE while Pauli noise (p1 or p2 > 0), shot noise or an amplitude shard is set on the handle, and in the
 * exact channel noise mode unless vqe_set_dm_grad(h, 1) and vqe_set_dm_batched(h, != 0) were called: then the batched
 * path computes the gradient of tr(rho H) for the channel of vqe_set_noise, whatever p1 / p2.  On a term-sharded
 * handle energy and gradient are the shard's partial sums. */
int vqe_energy_grad_batch(vqe_t* h, int batch, const double* theta /* batch x P */,
                          double* energy /* batch */, double* grad /* batch x P */);
/* replaces: circuit.update_quantum_state(state); state.get_vector()  (:84-85) */
int vqe_get_state(vqe_t* h, const double* theta, double* amps_re_im /* 2 * 2^n */);
/* replaces: scipy.optimize.minimize(cost, x0, method='COBYLA', options={'maxiter': m})
 * at environment_qulacs_TN_notin_agent.py:478 (scipy 1.15: rhobeg=1.0, rhoend=1e-4,
 * maxfun=m).  The whole loop (simplex algebra + evaluations) runs on the device. */
int vqe_minimize_cobyla(vqe_t* h, const double* x0, double rhobeg, double rhoend,
                        int maxfun, double* x, double* f, int32_t* nfev);

/* ---- batches of independent circuits (one per parallel environment / RL seed) ---------
 * Circuits are concatenated; circuit b owns gates [gate_off[b], gate_off[b+1]) and
 * parameters [par_off[b], par_off[b+1]); param_idx is local to the circuit.
 * vqe_batch_load copies the description (and x0 / theta) into device memory; the
 * *_run calls only launch device work on resident data and never modify it (a run can be
 * repeated); vqe_batch_fetch copies results back.  replaces: B independent CircuitEnv.scipy_optim / get_energy calls
 * (environment_qulacs_TN_notin_agent.py:442-482).
 * A handle holds ONE resident batch.  vqe_batch_load replaces it and clears the new gates of vqe_batch_set_new_gate
 * (an env-step after a load without a new vqe_batch_set_new_gate optimises the full circuits); a refused load
 * (VQE_EINVAL) leaves the previous batch, its new gates and its fetchable results as they were.  The one-circuit calls
 * (vqe_energy*, vqe_energy_grad_batch, vqe_get_state*, vqe_minimize_cobyla, vqe_minimize_lbfgs) load the circuit of
 * vqe_set_circuit as a batch of their own: after one of them the resident batch is THAT circuit (`batch` copies of it for
 * the *_batch calls), and vqe_batch_run_* / vqe_batch_fetch* serve it, not the batch loaded before - load again to go
 * back.  Results on the device (x, xopt, f, nfev, gradients, traces) belong to the last run: another run overwrites them. */
int vqe_batch_load(vqe_t* h, int batch, const int64_t* gate_off, const int32_t* kind,
                   const int32_t* q0, const int32_t* q1, const int32_t* param_idx,
                   const int64_t* par_off, const double* theta0);
int vqe_batch_run_energy(vqe_t* h);
int vqe_batch_run_minimize(vqe_t* h, double rhobeg, double rhoend, int maxfun);
/* streaming path (n >= 14): redo only the Pauli-term reduction <psi|H_shard|psi> on the
 * states left by the previous vqe_batch_run_energy (for timing the sharded reduction) */
int vqe_batch_run_reduction(vqe_t* h);
/* One CircuitEnv.step() worth of arithmetic per circuit, in ONE launch
 * (environment_qulacs_TN_notin_agent.py:283-291): new_gate[b] is the index, inside circuit
 * b, of the gate the RL action just added (-1: none).  COBYLA runs on the circuit WITHOUT
 * that gate from x0 = theta0 (the reference optimises the pre-action state, :453); the
 * optimum is rounded to float32 (state-tensor dtype, :480) and the energy of the FULL
 * circuit at those angles is returned in f (the extra get_energy() of :291).  x receives
 * all n_params angles (the new rotation keeps its theta0 value), nfev COBYLA's count.
 * A noise gate that directly follows gate new_gate[b] and acts on the same qubit(s) is the
 * channel construct_ansatz attached to it (VQE_qulacs_TN_notin_RL_noise.py:26-28,40-50) and is
 * left out of the optimised circuit with it; the noise draws of the COBYLA phase are numbered by
 * gate position in that pre-action circuit, those of the final evaluation by position in the
 * full one.  n <= 13: one fused launch; n >= 14 (streaming path): the same steps with the COBYLA loop
 * driven by the host over batched evaluations. */
int vqe_batch_set_new_gate(vqe_t* h, const int32_t* new_gate /* batch, or NULL */);
int vqe_batch_run_env_step(vqe_t* h, double rhobeg, double rhoend, int maxfun);
int vqe_batch_fetch(vqe_t* h, double* x /* sum of n_params, may be NULL */,
                    double* f /* batch */, int32_t* nfev /* batch, may be NULL */);
/* vqe_energy_grad_batch for the resident batch of vqe_batch_load (circuits of different lengths and parameter
 * counts): energies land where vqe_batch_run_energy puts them (vqe_batch_fetch's f), the gradients are copied back
 * by vqe_batch_fetch_grad in the layout of vqe_batch_fetch's x.  replaces: the finite-difference gradients of B
 * independent scipy.optimize.minimize calls with a gradient method (environment_qulacs_TN_notin_agent.py:452-482);
 * same n range and refusals as vqe_energy_grad_batch. */
int vqe_batch_run_energy_grad(vqe_t* h);
int vqe_batch_fetch_grad(vqe_t* h, double* grad /* sum of n_params, layout of vqe_batch_fetch's x */);
/* the optimiser's result before the float32 rounding of vqe_batch_run_env_step
 * (scipy's result.x, stored by the reference as env.opt_ang_save, :288); same layout as x.  After a run that rounds
 * nothing (vqe_batch_run_minimize, vqe_batch_run_minimize_lbfgs, on every path) it equals vqe_batch_fetch's x. */
int vqe_batch_fetch_xopt(vqe_t* h, double* x /* sum of n_params */);
/* ---- device L-BFGS on the adjoint gradient ---------------------------------------------------
 * A batched quasi-Newton optimiser with the shape of the COBYLA launch: one workgroup per circuit, and the whole loop -
 * energy + gradient (the adjoint sweep of vqe_energy_grad_batch), two-loop recursion over `history` pairs, Armijo
 * backtracking - inside ONE launch, no host round trip per iteration.  The cost of an iteration does not grow with the
 * number of parameters.
 * replaces: scipy.optimize.minimize(cost, x0, method='L-BFGS-B', jac=...) of
 * environment_qulacs_TN_notin_agent.py:452-482, B times - with this CAVEAT: it is NOT scipy's L-BFGS-B.  There are no
 * bounds, the line search is Armijo backtracking (t = 1, 1/2, 1/4, ...; accept f(x + t d) <= f + c1 t g.d) and not
 * More-Thuente, and the trajectories differ from scipy's.  CircuitEnv's optim_alg = "L-BFGS-B" keeps running scipy on
 * the host.  The algorithm, decision for decision, is in csrc/vqe_lbfgs.h and DESIGN 4.8.
 * status: 0 max|g_j| <= gtol; 1 f - f_new <= ftol max(|f|, |f_new|, 1); 2 no step accepted in max_ls trials (x, f
 * unchanged); 3 maxfun evaluations used; 4 maxiter accepted steps made.  x is always the best point (Armijo makes f
 * monotone).  Parameters that no gate uses never move.
 * 1 <= n <= 13: the one-launch kernel.  n >= 14: VQE_EINVAL unless vqe_set_stream_lbfgs(h, 1) was called; then the same
 * algorithm runs on the streaming path, all resident streams in lock-step: per evaluation the streaming adjoint gradient
 * and one small update kernel (csrc/vqe_stream_lbfgs.h), nothing copied to the host in between.  A
 * vqe_batch_run_reduction right after such a minimise run is refused with VQE_ESTATE (its last launch was a gradient);
 * after an env-step it is accepted.  Exact channel mode after vqe_set_dm_grad(h, 1) and vqe_set_dm_batched(h, != 0):
 * the same lock-step form on the batched density-matrix path (csrc/vqe_dm_grad.h), an env-step on the
 * pre-action circuits.  Refused with VQE_ESTATE, before anything is launched, while Pauli noise, the exact channel
 * mode without those two switches, shot noise, an amplitude shard or a term shard (the line search needs the full
 * energy) is set;
 * VQE_EINVAL for history outside 1..16, maxiter < 0, maxfun < 1, max_ls < 1, a negative tolerance or c1 outside (0, 1).
 * opts == NULL: the defaults. */
typedef struct { int32_t history; int32_t maxiter; int32_t maxfun; int32_t max_ls;
                 double gtol, ftol, c1; } vqe_lbfgs_opts_t;
/* replaces: the `options` dict of that scipy call (:478) */
int vqe_lbfgs_default_opts(vqe_lbfgs_opts_t* o);            /* 8, 100, 1000, 20, 1e-6, 1e-12, 1e-4 */
/* replaces: one such scipy.optimize.minimize call on the circuit of vqe_set_circuit (see the caveat above);
 * nit = accepted steps; nfev, nit, status may be NULL */
int vqe_minimize_lbfgs(vqe_t* h, const double* x0, const vqe_lbfgs_opts_t* opts, double* x, double* f,
                       int32_t* nfev, int32_t* nit, int32_t* status);
/* replaces: B such calls, on the resident batch from x0 = theta0 (see the caveat above).  vqe_batch_fetch,
 * vqe_batch_fetch_xopt, vqe_batch_energy_devptr, vqe_batch_copy_energy, vqe_last_kernel_ms and - after
 * vqe_batch_set_trace(1) - vqe_batch_fetch_trace serve these launches as they serve COBYLA's. */
int vqe_batch_run_minimize_lbfgs(vqe_t* h, const vqe_lbfgs_opts_t* opts);
/* replaces: B CircuitEnv.step() calls with a gradient optim_alg (environment_qulacs_TN_notin_agent.py:283-291,452-482;
 * see the caveat above): vqe_batch_run_env_step with the L-BFGS in COBYLA's place - it optimises the circuit WITHOUT
 * gate new_gate[b] (vqe_batch_set_new_gate), rounds the optimum to float32 and returns the energy of the FULL circuit
 * at those angles in f; the new rotation keeps its theta0 value. */
int vqe_batch_run_env_step_lbfgs(vqe_t* h, const vqe_lbfgs_opts_t* opts);
/* replaces: result.nit / result.status of those scipy calls (status numbered as above); either pointer may be NULL */
int vqe_batch_fetch_lbfgs_info(vqe_t* h, int32_t* nit /* batch */, int32_t* status /* batch */);
/* ---- device Adam-SPSA: a two-evaluation optimiser for stochastic energies -------------------------
 * replaces: nothing in the reference - its configs carry the [non_local_opt] keys a, alpha, c, gamma, lamda, beta_1,
 * beta_2, but no code path of it reads them.  Simultaneous-perturbation gradient estimates fed to Adam, the whole loop
 * in one launch, one workgroup per circuit (csrc/vqe_spsa.h; the update of an element and the schedule: csrc/spsa_m0.h;
 * DESIGN 4.22).  With K = maxiter, P parameters and `hole` the new gate's angle of an env-step (or none):
 *   x = x0;  m = v = 0;  b1p = b2p = 1
 *   for k = 0 .. K-1:
 *       a_k = a / (k + 1 + stability)^alpha;   c_k = c / (k + 1)^gamma
 *       key = noise_key(seed, b, k)                              (the engine's counter RNG; b = position in the batch)
 *       D_j = +1 if noise_uniform_k(key, j) < 0.5 else -1        (j = 0 .. P-1; D_hole = 0)
 *       f+ = E(x + c_k D), evaluation id eval_base + 2k;   f- = E(x - c_k D), evaluation id eval_base + 2k + 1
 *       g_j = (f+ - f-) / (2 c_k) * D_j
 *       b1k = beta_1 / (k + 1)^lamda
 *       m = b1k m + (1 - b1k) g;   v = beta_2 v + (1 - beta_2) g*g;   b1p *= b1k;   b2p *= beta_2
 *       x_j -= a_k * (m_j / (1 - b1p)) / (sqrt(v_j / (1 - b2p)) + eps)
 * E is the handle's mode 0 energy: noiseless, or one draw of the Pauli errors (vqe_set_noise / vqe_set_noise_pauli) keyed
 * by the evaluation id, plus the shot-noise term of vqe_set_shot_noise - what the device COBYLA evaluates.  `seed` is the
 * seed of the perturbations alone (not the noise seed): the optimiser runs on a handle without noise.
 * Plain minimise: one more evaluation f = E(x_K), id eval_base + 2K; nfev = 2K + 1; x and xopt are x_K.
 * Env-step: the loop runs on the circuit WITHOUT gate new_gate[b], the new rotation keeps its theta0 value, x is x_K
 * rounded through float32 and f the energy of the FULL circuit there, id eval_base + 2K; nfev = 2K (the closing
 * evaluation is not counted, as with the other two optimisers).
 * K = 0, or a circuit without an optimised parameter: that closing evaluation alone, id eval_base, nfev = 1.
 * After a run eval_base has advanced by 2K + 1.  The results have the same bits for the same (seed, b, noise seed,
 * eval_base), whatever the batch size and the other circuits.
 * VQE_EINVAL before anything is launched (the handle stays usable): a non-finite option, maxiter < 0, a <= 0, c <= 0,
 * eps <= 0, alpha / gamma / lamda / stability < 0, beta_1 or beta_2 outside [0, 1); n_qubits >= 14.
 * VQE_ESTATE: the exact channel mode (vqe_set_noise_mode 1), a Kraus override (with or without vqe_set_kraus_traj),
 * term- and amplitude-sharded handles.  A refused call changes nothing, eval_base included.
 * opts == NULL on vqe_minimize_spsa / vqe_batch_run_*_spsa: VQE_EINVAL (the shipped configs carry no usable defaults;
 * start from vqe_spsa_default_opts). */
typedef struct { int32_t maxiter; double a, alpha, stability, c, gamma, beta_1, beta_2, lamda, eps;
                 uint64_t seed; } vqe_spsa_opts_t;
int vqe_spsa_default_opts(vqe_spsa_opts_t* o);             /* 100, 0.1, 0.602, 0, 0.1, 0.101, 0.9, 0.999, 0, 1e-8, 0 */
/* one such run on the circuit of vqe_set_circuit; nfev may be NULL */
int vqe_minimize_spsa(vqe_t* h, const double* x0, const vqe_spsa_opts_t* opts, double* x, double* f, int32_t* nfev);
/* B such runs on the resident batch from x0 = theta0.  vqe_batch_fetch, vqe_batch_fetch_xopt, vqe_batch_energy_devptr,
 * vqe_batch_copy_energy, vqe_last_kernel_ms and - after vqe_batch_set_trace(1) - vqe_batch_fetch_trace serve these
 * launches as they serve COBYLA's; the trace holds 2K + 1 rows (evaluation e in row e; an env-step leaves row 2K zero). */
int vqe_batch_run_minimize_spsa(vqe_t* h, const vqe_spsa_opts_t* opts);
int vqe_batch_run_env_step_spsa(vqe_t* h, const vqe_spsa_opts_t* opts);
/* ---- device Lanczos: the extreme eigenpair of the Hamiltonian ------------------------------------
 * The lowest (which = 0) or highest (which = 1) eigenvalue of the handle's Hamiltonian and its eigenvector, by Lanczos
 * on the device: a stored basis of at most max_basis vectors (complex128[2^n] each, in global memory; fewer when 2^n
 * or a quarter of the free device memory holds fewer beside three work vectors - VQE_ENOMEM below 2), full
 * reorthogonalisation, explicit restart from the current Ritz vector when the basis is full.  Every step is queued on
 * the handle's stream; the host reads the recurrence coefficients every check_every steps and stops when the residual
 * estimate is <= tol * max(1, |theta|).  The same path for every n the handle accepts (csrc/vqe_lanczos.h).
 * replaces: numpy.linalg.eigvalsh of the dense operator - the `eigvals` of the reference's Hamiltonian files, whose
 * minimum is the environments' min_eig (environment_qulacs_TN_notin_agent.py:126-131,166-167) - and the DMRG run whose
 * state the init circuit is fitted to; the reference ships neither for its 12- and 20-qubit problems.
 * THE KRYLOV LIMIT: the result is the extreme eigenpair of H restricted to the Krylov space of the start vector.  The
 * default start (uniform draws from `seed`) overlaps every eigenvector; with start_from_init the start is the handle's
 * initial state, and a start without a component along the wanted eigenvector never finds it - from an exact
 * eigenvector the answer is that eigenvector after one application, whatever its place in the spectrum.
 * *eigenvalue is the Rayleigh quotient of the returned vector (never below the true minimum), amps the normalised
 * vector (NULL: not copied; the _dev variant takes device memory, complex128[2^n], and returns the same bits).
 * info = {true residual |H y - theta y|, H applications of the recurrence, restarts, status}; status 0 converged,
 * 1 breakdown (the Krylov space is an exact invariant subspace: the pair is exact in it), 2 max_matvec applications
 * used up - NOT an error: VQE_OK with the best Ritz pair so far and its true residual.  Two calls with equal options
 * return equal bits.
 * Refused before anything is launched, handle unchanged: VQE_ESTATE without a Hamiltonian, on a term shard with
 * world > 1 (a shard's spectrum is not H's) or an amplitude shard; VQE_EINVAL for which outside {0, 1}, max_basis < 2,
 * max_matvec < 1, check_every < 1, tol <= 0 or not finite.  Noise settings and the circuit play no part; the call
 * changes neither the initial state, the resident batch and its results, the noise counter nor any later result of
 * the handle.  vqe_last_kernel_ms reports the run. */
typedef struct { int32_t which;          /* 0 lowest, 1 highest */
                 int32_t max_basis, max_matvec, check_every, start_from_init;
                 double tol; uint64_t seed; } vqe_lanczos_opts_t;
int vqe_lanczos_default_opts(vqe_lanczos_opts_t* o);   /* 0, 128, 2000, 8, 0, 1e-10, 1 */
int vqe_lanczos(vqe_t* h, const vqe_lanczos_opts_t* opts /* NULL: defaults */, double* eigenvalue,
                double* amps_re_im /* 2 * 2^n or NULL */, double info[4]);
int vqe_lanczos_dev(vqe_t* h, const vqe_lanczos_opts_t* opts, double* eigenvalue,
                    void* dev_amps_re_im /* or NULL */, double info[4]);
/* ---- device Lanczos: several eigenpairs, with multiplicities ------------------------------------------
 * The n_eig lowest (which = 0) or highest (which = 1) eigenpairs of the handle's Hamiltonian, copies of a degenerate
 * eigenvalue included: thick-restart Lanczos with locking by deflation, one stage per pair.  Stage e draws
 * a fresh random start vector (from seed and e; stage 0 has the start vector of vqe_lanczos) orthogonal to the e vectors
 * found so far, which stay in the basis storage, so the full reorthogonalisation of every step keeps the recurrence in
 * their complement.  A full active basis keeps `keep` Ritz vectors and the residual vector and goes on (keep = 0: the
 * library's rule, half the active basis; with fewer than 3 active vectors: the explicit restart of vqe_lanczos).  A stage
 * ends by the stop rule of vqe_lanczos.  Storage: max_basis + n_eig - 1 vectors beside the three work vectors, fewer when
 * 2^n or a quarter of the free device memory holds fewer - stage e then has min(max_basis, slots - e, 2^n - e, 1024)
 * active vectors; VQE_ENOMEM, before anything is launched, if the last stage would have fewer than 2 (1 where a single
 * dimension is left).
 * replaces: the low (high) end of numpy.linalg.eigvalsh of the dense operator - the `eigvals` array of the reference's
 * Hamiltonian files - where the dense matrix cannot exist, with the gap and the degeneracy of the ground level.
 * eigenvalues[i] ascend for which = 0 and descend for which = 1, each the Rayleigh quotient of vector i; amps holds the
 * normalised vectors one after the other (n_eig x 2 * 2^n doubles; NULL: not copied; the _dev variant takes device
 * memory and returns the same bits); residuals[i] = |H y_i - theta_i y_i|.  max_matvec counts the H applications of all
 * stages together.  info = {largest true residual, H applications of the recurrences, restarts, status, pairs returned}:
 * status 0 all pairs converged, 1 some stage ended at a breakdown (its pair is exact in its space), 2 max_matvec spent -
 * NOT an error: VQE_OK with the pairs found so far (info[4] of them; the other entries of eigenvalues and residuals are
 * NaN, their vectors are not written).  Two calls with equal options return equal bits.
 * THE KRYLOV LIMIT, as for vqe_lanczos: pair e is extreme in the Krylov space of a random vector orthogonal to the
 * locked vectors, for H restricted to their complement; the locked vectors are eigenvectors only up to their reported
 * residuals, which bounds what the later pairs can inherit from them.
 * Refused before anything is launched, handle unchanged: as vqe_lanczos (no Hamiltonian, term shard, amplitude shard,
 * which, max_basis < 2, max_matvec < 1, check_every < 1, tol), and VQE_EINVAL for n_eig outside 1 .. min(2^n, 64),
 * keep < 0 or keep >= max_basis - 1.  The call changes neither the initial state, the resident batch and its results,
 * the noise counter nor any later result of the handle.  vqe_last_kernel_ms reports the run. */
typedef struct { int32_t which, n_eig, max_basis, max_matvec, check_every, keep;  /* keep 0: the library's rule */
                 double tol; uint64_t seed; } vqe_lanczos_multi_opts_t;
int vqe_lanczos_multi_default_opts(vqe_lanczos_multi_opts_t* o);   /* 0, 1, 128, 2000, 8, 0, 1e-10, 1 */
int vqe_lanczos_multi(vqe_t* h, const vqe_lanczos_multi_opts_t* opts /* NULL: defaults */, double* eigenvalues /* n_eig */,
                      double* amps_re_im /* n_eig x 2 * 2^n or NULL */, double* residuals /* n_eig */, double info[5]);
int vqe_lanczos_multi_dev(vqe_t* h, const vqe_lanczos_multi_opts_t* opts, double* eigenvalues,
                          void* dev_amps_re_im /* or NULL */, double* residuals, double info[5]);
/* device pointer to the batch's f / energy array (float64[batch]) for on-device
 * reductions by the caller (e.g. torch.distributed all_reduce over RCCL) */
int vqe_batch_energy_devptr(vqe_t* h, void** dev_ptr);
/* asynchronous device-to-device copy of that array into caller-owned device memory
 * (e.g. a torch tensor) on the handle's stream */
int vqe_batch_copy_energy(vqe_t* h, void* dst_dev /* float64[batch] */);
/* Diagnostic: record (f, x[0..P)) of every COBYLA evaluation of the next vqe_batch_run_minimize /
 * vqe_batch_run_env_step launches (LDS-resident path), for trajectory-level comparison with
 * scipy's callback sequence (environment_qulacs_TN_notin_agent.py:464-468,478).
 * vqe_batch_fetch_trace copies circuit b's records: out[k * stride] = f of evaluation k + 1,
 * out[k * stride + 1 + j] = its trial point (the optimised parameters only: the new gate's angle is
 * not among them), zero beyond nfev; out == NULL only queries maxfun / stride. */
int vqe_batch_set_trace(vqe_t* h, int enable);
int vqe_batch_fetch_trace(vqe_t* h, int circuit, double* out /* maxfun * stride, or NULL */,
                          int32_t* maxfun, int32_t* stride);
/* diagnostic builds only (-DVQE_STAMPS): [0] evaluations, [1] cycles in the circuit phase,
 * [2] in the energy phase, [3] in the optimiser update, summed over workgroups; read and
 * cleared.  All zero in the shipped library (no stamp executes there). */
int vqe_debug_counters(vqe_t* h, uint64_t out[8]);
/* kernel time of the last *_run call measured with HIP events on the handle's stream */
int vqe_last_kernel_ms(vqe_t* h, float* ms);

/* ---- host-side COBYLA (ask/tell) -------------------------------------------------------
 * Same algorithm as the device loop; used when every evaluation needs a collective
 * (Pauli-term sharding across GPUs) or by a caller with its own cost function.
 * replaces: scipy.optimize.minimize(..., method='COBYLA') as above. */
int vqe_cobyla_create(int n, const double* x0, double rhobeg, double rhoend, int maxfun,
                      vqe_cobyla_t** out);
/* returns 1 and fills x[n] when f(x) is wanted, 0 when finished, <0 on error */
int vqe_cobyla_ask(vqe_cobyla_t* c, double* x);
int vqe_cobyla_tell(vqe_cobyla_t* c, double f);
int vqe_cobyla_result(vqe_cobyla_t* c, double* x, double* f, int32_t* nfev, int32_t* status);
void vqe_cobyla_destroy(vqe_cobyla_t* c);

#ifdef __cplusplus
}
#endif
#endif /* VQE_HIP_H */
