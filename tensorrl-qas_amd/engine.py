"""numpy-facing wrapper of the C ABI (include/vqe_hip.h).  Thin: argument marshalling and
error translation only; all arithmetic happens in libvqe_hip.so on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import VQEError, c_f64p, c_i32p, c_i64p, c_u64p

GATE_CNOT, GATE_RX, GATE_RY, GATE_RZ, GATE_DEPOL1, GATE_DEPOL2 = range(6)
# two-qubit Pauli rotations exp(+i theta/2 P_q0 P_q1) of the SU(4) gate set (reference VQE_qulacs_su4.py:68-90)
GATE_RXX, GATE_RYY, GATE_RZZ = 6, 7, 8


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None and a.size else C.cast(None, t)


class Circuit:
    """Gate list in construct_ansatz order (reference VQE_qulacs_TN_notin_RL.py:13-45):
    parallel int32 arrays ``kind, q0, q1, pidx`` and the number of parameters.  RXX / RYY / RZZ
    (VQE_qulacs_su4.py:13-45) take two distinct qubits and a parameter index."""

    # ``angles``: optional parameter values carried by the handle (the reference's qulacs
    # circuit holds its parameters; the VQAs shim uses this)
    __slots__ = ("kind", "q0", "q1", "pidx", "n_params", "angles")

    def __init__(self, kind, q0, q1, pidx, n_params):
        self.kind, self.q0, self.q1, self.pidx = _i32(kind), _i32(q0), _i32(q1), _i32(pidx)
        self.n_params = int(n_params)
        self.angles = None

    def __len__(self):
        return int(self.kind.size)

    @staticmethod
    def empty():
        z = np.zeros(0, np.int32)
        return Circuit(z, z, z, z, 0)


COBYLA_CLASSES = ("resident", "staged", "global", "rows", "block")      # VQE_COBYLA_* of include/vqe_hip.h


def _placement(out):
    return {"class": COBYLA_CLASSES[out[0]], "pad": int(out[1]), "words": int(out[2]), "lds_bytes": int(out[3]),
            "split": bool(out[4]), "tile_bytes": int(out[5]), "resident_bytes": int(out[6]), "accepted": bool(out[7])}


def cobyla_placement(n_qubits, max_ops, max_pair, max_params, n_groups, n_params, wide):
    """vqe_cobyla_placement (host only): what a minimiser launch of the LDS-resident kernels with these batch sizes
    does with the optimiser's arrays of a circuit of ``n_params`` parameters - the kernel's own decision function.
    -> dict(class, pad, words, lds_bytes, split, tile_bytes, resident_bytes, accepted)"""
    out = (C.c_int64 * 8)()
    rc = _lib.load().vqe_cobyla_placement(int(n_qubits), int(max_ops), int(max_pair), int(max_params), int(n_groups),
                                          int(n_params), int(bool(wide)), out)
    if rc != 0:
        raise ValueError("vqe_cobyla_placement: argument out of range")
    return _placement(out)


def pair_lds_plan(n_qubits, max_ops, max_pair, max_params, n_groups):
    """vqe_pair_lds_plan (host only): the LDS layout of a paired minimiser launch with these batch sizes."""
    out = (C.c_int64 * 12)()
    rc = _lib.load().vqe_pair_lds_plan(int(n_qubits), int(max_ops), int(max_pair), int(max_params), int(n_groups), out)
    if rc != 0:
        raise ValueError("vqe_pair_lds_plan: argument out of range")
    names = ("sched", "lay", "cs", "xm", "zm", "meta", "sb", "sidx", "rec", "bytes", "single_bytes", "state_bytes")
    return {k: int(v) for k, v in zip(names, out)}


class VQEEngine:
    """One handle = one (n_qubits, initial state, Hamiltonian) problem on one GPU."""

    def __init__(self, n_qubits: int, device_id: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.n_qubits = int(n_qubits)
        rc = self._lib.vqe_create(self.n_qubits, int(device_id), C.byref(self._h))
        if rc:
            msg = self._lib.vqe_last_error(None)
            self._h = C.c_void_p()
            raise VQEError(f"vqe_create failed ({rc}): {msg.decode() if msg else ''}")
        self._batch = 0
        self._traj_rows = 0      # the rows of batch_fetch_traj: the circuits of the last energy call / batch load that
                                 # succeeded, and never fewer than the library's resident batch (a call that fails may
                                 # or may not have loaded its batch: the count only grows until one succeeds)
        self._total_params = 0

    # -- plumbing -------------------------------------------------------------------------
    def _chk(self, rc):
        if rc:
            msg = self._lib.vqe_last_error(self._h)
            raise VQEError(f"libvqe_hip error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.vqe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int | None):
        self._chk(self._lib.vqe_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def get_stream(self) -> int:
        """The HIP stream the handle issues its work on (as an integer pointer)."""
        p = C.c_void_p()
        self._chk(self._lib.vqe_get_stream(self._h, C.byref(p)))
        return int(p.value or 0)

    def sync(self):
        self._chk(self._lib.vqe_sync(self._h))

    def device_info(self):
        info = (C.c_int64 * 4)()
        self._chk(self._lib.vqe_device_info(self._h, info))
        return {"cu_count": info[0], "lds_per_cu": info[1], "wg_per_cu": info[2], "lds_path": bool(info[3])}

    # -- problem --------------------------------------------------------------------------
    def set_init_state(self, psi):
        if psi is None:
            self._chk(self._lib.vqe_set_init_state(self._h, C.cast(None, c_f64p)))
            return
        a = np.ascontiguousarray(psi, dtype=np.complex128)
        if a.size != 1 << self.n_qubits:
            raise ValueError("initial state has the wrong length")
        self._chk(self._lib.vqe_set_init_state(self._h, a.view(np.float64).ctypes.data_as(c_f64p)))

    def set_init_state_dev(self, dev_ptr: int):
        """Initial state from device memory (complex128[2^n]); asynchronous on the handle's stream."""
        self._chk(self._lib.vqe_set_init_state_dev(self._h, C.c_void_p(int(dev_ptr))))

    def get_state_dev(self, theta, dev_ptr: int):
        """U(theta)|init> written to device memory (complex128[2^n]); asynchronous on the handle's stream."""
        th = _f64(theta)
        if th.size != self._P:
            raise ValueError("theta has the wrong length")
        self._chk(self._lib.vqe_get_state_dev(self._h, _p(th, c_f64p), C.c_void_p(int(dev_ptr))))

    def set_hamiltonian(self, xmask, zmask, coeff):
        x = np.ascontiguousarray(xmask, dtype=np.uint64)
        z = np.ascontiguousarray(zmask, dtype=np.uint64)
        c = _f64(coeff)
        if not (x.size == z.size == c.size):
            raise ValueError("xmask, zmask, coeff differ in length")
        self._chk(self._lib.vqe_set_hamiltonian_pauli(self._h, int(x.size), _p(x, c_u64p), _p(z, c_u64p), _p(c, c_f64p)))

    def set_hamiltonian_dense(self, op, tol: float = 1e-13):
        """Dense operator in the simulator's little-endian basis (what the reference passes to
        get_exp_val); decomposed into Pauli terms by the library.  Returns (n_terms, n_xgroups)."""
        a = np.ascontiguousarray(op, dtype=np.complex128)
        dim = 1 << self.n_qubits
        if a.shape != (dim, dim):
            raise ValueError("operator has the wrong shape")
        self._chk(self._lib.vqe_set_hamiltonian_dense(self._h, a.view(np.float64).ctypes.data_as(c_f64p), float(tol)))
        nt, ng = C.c_int32(), C.c_int32()
        self._chk(self._lib.vqe_hamiltonian_terms(self._h, C.byref(nt), C.byref(ng)))
        return nt.value, ng.value

    def hamiltonian_terms(self):
        """(n_terms, n_xgroups) of the Hamiltonian as the library holds it."""
        nt, ng = C.c_int32(), C.c_int32()
        self._chk(self._lib.vqe_hamiltonian_terms(self._h, C.byref(nt), C.byref(ng)))
        return nt.value, ng.value

    def hamiltonian_layout(self):
        """How the LDS-resident kernels hold the Hamiltonian: table groups, units (mostly-zero groups), class groups."""
        out = (C.c_int32 * 4)()
        self._chk(self._lib.vqe_hamiltonian_layout(self._h, out))
        return {"table_groups": out[0], "units": out[1], "class_groups": out[2], "has_diag": bool(out[3])}

    def batch_cobyla_placement(self, circuit: int):
        """Where the device COBYLA keeps the arrays of circuit ``circuit`` of the resident batch and which of its
        contexts updates them (n <= 13; see cobyla_placement)."""
        out = (C.c_int64 * 8)()
        self._chk(self._lib.vqe_batch_cobyla_placement(self._h, int(circuit), out))
        return _placement(out)

    def unit_bank_score(self):
        """Modelled LDS bank conflicts of the unit path: mean / worst lanes per 16-byte slot of a ds_read_b128 lane group
        with the plain state layout ("plain_*") and with the bank swizzle this handle uses (1.0 = conflict free)."""
        out = (C.c_double * 4)()
        self._chk(self._lib.vqe_unit_bank_score(self._h, out))
        return {"plain_mean": out[0], "plain_worst": out[1], "mean": out[2], "worst": out[3]}

    # -- RCCL behind the C ABI (the collective of the term-sharded sum as a library call) -----------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = _lib.load().vqe_comm_unique_id(buf)
        if rc:
            raise VQEError(f"vqe_comm_unique_id failed ({rc})")
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._lib.vqe_comm_init(self._h, int(rank), int(world), buf))

    def comm_allreduce_energy(self):
        self._chk(self._lib.vqe_comm_allreduce_energy(self._h))

    def comm_destroy(self):
        self._chk(self._lib.vqe_comm_destroy(self._h))

    def set_term_shard(self, rank: int, world: int):
        self._chk(self._lib.vqe_set_term_shard(self._h, int(rank), int(world)))

    def set_amplitude_shard(self, rank: int, world: int):
        self._chk(self._lib.vqe_set_amplitude_shard(self._h, int(rank), int(world)))

    def set_stream_grad(self, enable: bool = True):
        """n >= 14: let energy_grad / energy_grad_batch / batch_run_energy_grad run on the streaming path (one more
        state-sized buffer per resident stream).  Off by default: those calls then raise at n >= 14.  No effect at
        n <= 13."""
        self._chk(self._lib.vqe_set_stream_grad(self._h, 1 if enable else 0))

    def set_stream_lbfgs(self, enable: bool = True):
        """n >= 14: let minimize_lbfgs / batch_run_minimize_lbfgs / batch_run_env_step_lbfgs run on the streaming path
        (all resident streams in lock-step, one adjoint gradient per evaluation; one more state-sized buffer per
        resident stream).  Off by default: those calls then raise at n >= 14, whatever set_stream_grad says.  No
        effect at n <= 13."""
        self._chk(self._lib.vqe_set_stream_lbfgs(self._h, 1 if enable else 0))

    def set_env_pairing(self, enable: bool = True):
        """10 <= n <= 13: let batch_run_minimize / batch_run_env_step put two environments into one workgroup where
        the launch allows it (vqe_set_env_pairing).  On by default; the results are those of the unpaired launch, bit
        for bit."""
        self._chk(self._lib.vqe_set_env_pairing(self._h, 1 if enable else 0))

    def last_env_pairing(self):
        """What the last launch of an LDS-resident kernel did (vqe_last_env_pairing)."""
        out = (C.c_int64 * 4)()
        self._chk(self._lib.vqe_last_env_pairing(self._h, out))
        return {"paired": bool(out[0]), "pairs": int(out[1]), "singles": int(out[2]), "lds_bytes": int(out[3])}

    def set_noise(self, p1: float, p2: float, seed: int):
        self._chk(self._lib.vqe_set_noise(self._h, float(p1), float(p2), C.c_uint64(int(seed) & (2 ** 64 - 1))))

    def set_noise_mode(self, mode: int):
        """0: Pauli trajectories (one draw per evaluation); 1: the exact channel (density matrix, n <= 13)."""
        self._chk(self._lib.vqe_set_noise_mode(self._h, int(mode)))

    def noise_mode_info(self):
        out = (C.c_int32 * 2)()
        self._chk(self._lib.vqe_noise_mode_info(self._h, out))
        return {"mode": out[0], "blocks_last_evaluation": out[1]}

    def set_dm_batched(self, max_resident: int = -1):
        """Exact channel mode (set_noise_mode(1)): evaluate the resident batch in lock-step on the device, COBYLA of
        minimize_cobyla / batch_run_minimize / batch_run_env_step on the device too.  ``max_resident``: density matrices
        held at a time - 0 the serial host-driven path (default of a new engine), -1 what fits a quarter of the free
        device memory, R >= 1 at most R (a batch larger than that is evaluated in chunks)."""
        self._chk(self._lib.vqe_set_dm_batched(self._h, int(max_resident)))

    def set_dm_grad(self, enable: bool = True):
        """Exact channel mode on the batched path (set_noise_mode(1) + set_dm_batched): let energy_grad /
        energy_grad_batch / batch_run_energy_grad and minimize_lbfgs / batch_run_minimize_lbfgs /
        batch_run_env_step_lbfgs run there, on the adjoint gradient of tr(rho H).  Off by default: those calls raise in
        mode 1.  A resident circuit then costs levels + 2 density matrices (dm_batch_info reports the resident count)."""
        self._chk(self._lib.vqe_set_dm_grad(self._h, 1 if enable else 0))

    def set_noise_kraus(self, K1=None, K2=None):
        """Exact channel mode: Kraus sets in the two noise slots (see ``channels``).  ``K1``: (k, 2, 2) complex, applied
        at GATE_DEPOL1 gates in the depolarising channel's place; ``K2``: (k, 4, 4) complex for GATE_DEPOL2, basis index
        = bit(q0) + 2 bit(q1) of the gate's two qubits.  ``None`` (or an empty set) leaves that slot on the depolarising
        channel of set_noise; both ``None`` removes the override.  While one is installed only mode 1 runs are served:
        mode 0 runs and get_state* raise, unless set_kraus_traj switched the quantum-jump trajectories on."""
        def pack(K, d, name):
            if K is None:
                return 0, None
            a = np.ascontiguousarray(K, dtype=np.complex128)
            if a.size == 0:
                return 0, None
            if a.ndim != 3 or a.shape[1:] != (d, d):
                raise ValueError(f"{name} must have shape (k, {d}, {d})")
            return int(a.shape[0]), a.view(np.float64)
        n1, a1 = pack(K1, 2, "K1")
        n2, a2 = pack(K2, 4, "K2")
        self._chk(self._lib.vqe_set_noise_kraus(self._h, n1, _p(a1, c_f64p), n2, _p(a2, c_f64p)))

    def noise_kraus_info(self):
        """Kraus operators installed in the one- / two-qubit slot (0: that slot runs the depolarising channel)."""
        out = (C.c_int32 * 2)()
        self._chk(self._lib.vqe_noise_kraus_info(self._h, out))
        return {"n1": out[0], "n2": out[1]}

    def set_noise_pauli(self, w1=None, w2=None):
        """Pauli channels in the two noise slots, drawn by the mode 0 sampler itself (one Pauli per gate and evaluation,
        as qulacs samples BitFlipNoise, DephasingNoise, IndependentXZNoise).  ``w1``: 3 probabilities of X, Y, Z at
        GATE_DEPOL1 gates; ``w2``: 15 probabilities of the codes ``a | b << 2`` (a on q0, b on q1, 1 = X, 2 = Y, 3 = Z)
        at GATE_DEPOL2 gates; ``channels.pauli_weights`` / ``channels.pauli_twirl`` make them from a Kraus set.  ``None``
        leaves that slot on the depolarising channel of set_noise; both ``None`` removes the tables.  Mode 1 and the
        quantum-jump runs use the same channel; a Kraus override (set_noise_kraus) on a slot wins over its table."""
        def pack(w, m, name):
            if w is None:
                return None
            a = np.ascontiguousarray(w, dtype=np.float64)
            if a.shape != (m,):
                raise ValueError(f"{name} must hold {m} probabilities")
            return a
        a1, a2 = pack(w1, 3, "w1"), pack(w2, 15, "w2")
        self._chk(self._lib.vqe_set_noise_pauli(self._h, _p(a1, c_f64p), _p(a2, c_f64p)))

    def noise_pauli_info(self):
        """Whether a Pauli table is installed in the one- / two-qubit slot (False: the depolarising channel)."""
        out = (C.c_int32 * 2)()
        self._chk(self._lib.vqe_noise_pauli_info(self._h, out))
        return {"w1": bool(out[0]), "w2": bool(out[1])}

    def set_noise_grad(self, n_real: int, hold: bool = False):
        """Mode 0 Pauli noise (set_noise p1 / p2 or set_noise_pauli): serve energy_grad* and the device L-BFGS at
        n <= 13 (at 14 <= n <= 20 after set_stream_noise_grad) on the mean over ``n_real`` frozen realisations - the draws batch_run_energy makes for the evaluation
        ids eval_base .. eval_base + n_real - 1 (1 .. 4096; 0, the default, leaves those calls refused).  A gradient
        run moves the counter on by n_real unless ``hold``: then it stays, a host optimiser sees one deterministic
        function, and noise_grad_advance() moves it.  An L-BFGS run always moves it (an env-step by n_real + 1: its
        closing energy is one more draw).  The definition: include/vqe_hip.h."""
        self._chk(self._lib.vqe_set_noise_grad(self._h, int(n_real), 1 if hold else 0))

    def noise_grad_advance(self):
        """Move the evaluation counter on by the n_real of set_noise_grad (fresh realisations for the next run)."""
        self._chk(self._lib.vqe_noise_grad_advance(self._h))

    def noise_grad_info(self):
        out = (C.c_int64 * 4)()
        self._chk(self._lib.vqe_noise_grad_info(self._h, out))
        return {"n_real": out[0], "hold": bool(out[1]), "eval_base": out[2]}

    def set_stream_noise_grad(self, max_resident: int = -1):
        """The gradients of set_noise_grad at 14 <= n <= 20 (the streaming path), opt-in per handle: every (circuit,
        realisation) pair is a stream of the adjoint sweeps (two states of 16 * 2^n bytes), ``max_resident`` of them
        at a time (-1: as many as fit into a quarter of the free device memory at the first run; 0: off, the calls are
        refused as before).  energy_grad* also needs set_stream_grad, the L-BFGS calls set_stream_lbfgs.  The bits of a
        result do not depend on it.  No effect at n <= 13."""
        self._chk(self._lib.vqe_set_stream_noise_grad(self._h, int(max_resident)))

    def stream_noise_grad_info(self):
        """max_resident as set, and of the last noisy gradient / L-BFGS run on the streaming path (0 before one) the
        pairs resident per chunk and the chunks per evaluation."""
        out = (C.c_int64 * 4)()
        self._chk(self._lib.vqe_stream_noise_grad_info(self._h, out))
        return {"max_resident": out[0], "resident": out[1], "chunks": out[2]}

    def set_kraus_traj(self, n_traj: int):
        """Mode 0 under a Kraus override (set_noise_kraus): evaluate an energy as the mean of ``n_traj`` quantum-jump
        trajectories (1 .. 4096; 0, the default, leaves those runs refused).  Served: energy / energy_batch /
        batch_run_energy, minimize_cobyla / batch_run_minimize / batch_run_env_step (COBYLA on the device, in
        lock-step) and get_state* (the normalised state of trajectory 0); unsharded handles, n <= 13 on the
        LDS-resident path and n >= 14 on the streaming path once set_stream_kraus_traj switched it on.  Gradient,
        L-BFGS and reduction calls stay refused.  The definition of a trajectory: include/vqe_hip.h."""
        self._chk(self._lib.vqe_set_kraus_traj(self._h, int(n_traj)))

    def set_stream_kraus_traj(self, max_resident: int = -1):
        """Quantum-jump trajectories at n >= 14 (the streaming path), opt-in per handle: every (circuit, trajectory)
        pair is a state of 16 * 2^n bytes in device memory, ``max_resident`` of them at a time (-1: as many as fit
        into a quarter of the free device memory at the first run; 0: off, the runs are refused as before).  The bits
        of an energy do not depend on it.  No effect at n <= 13."""
        self._chk(self._lib.vqe_set_stream_kraus_traj(self._h, int(max_resident)))

    def stream_kraus_traj_info(self):
        """The last trajectory run on the streaming path (all 0 before one): states resident per chunk, chunks per
        evaluation, jump rounds, state sweeps launched per chunk and evaluation ahead of the energy."""
        out = (C.c_int64 * 4)()
        self._chk(self._lib.vqe_stream_kraus_traj_info(self._h, out))
        return {"resident": out[0], "chunks": out[1], "rounds": out[2], "sweeps": out[3]}

    def kraus_traj_info(self):
        """The trajectory count and the last trajectory run: workgroups of its last launch, jumps (selections k != 0)
        of its last evaluation summed over circuits and trajectories, lock-step evaluations (1 for an energy run)."""
        out = (C.c_int64 * 4)()
        self._chk(self._lib.vqe_kraus_traj_info(self._h, out))
        return {"n_traj": out[0], "workgroups": out[1], "jumps": out[2], "evaluations": out[3]}

    def batch_fetch_traj(self) -> np.ndarray:
        """(batch, n_traj) per-trajectory energies of the last energy run, or of the final full-circuit evaluation of
        the last env-step; raises after anything else."""
        info = self.kraus_traj_info()
        out = np.empty((max(1, self._traj_rows), max(1, int(info["n_traj"]))), np.float64)
        self._chk(self._lib.vqe_batch_fetch_traj(self._h, _p(out, c_f64p)))
        return out

    def set_dm_rot2(self, enable: bool = True):
        """Exact channel mode: take GATE_RXX / RYY / RZZ as members of the superoperator blocks (serial and batched path,
        gradient and L-BFGS included).  Off by default: circuits with those gates are refused in mode 1."""
        self._chk(self._lib.vqe_set_dm_rot2(self._h, 1 if enable else 0))

    def dm_batch_info(self):
        """The last batched exact-channel run (all 0 after a serial one)."""
        out = (C.c_int64 * 4)()
        self._chk(self._lib.vqe_dm_batch_info(self._h, out))
        return {"resident": out[0], "chunks": out[1], "evaluations": out[2], "levels": out[3]}

    def set_shot_noise(self, sigma_total: float, seed: int):
        self._chk(self._lib.vqe_set_shot_noise(self._h, float(sigma_total), C.c_uint64(int(seed) & (2 ** 64 - 1))))

    # -- single circuit -------------------------------------------------------------------
    def set_circuit(self, circ: Circuit):
        self._P = circ.n_params
        self._chk(self._lib.vqe_set_circuit(self._h, len(circ), _p(circ.kind, c_i32p), _p(circ.q0, c_i32p),
                                            _p(circ.q1, c_i32p), _p(circ.pidx, c_i32p), circ.n_params))

    def energy(self, theta) -> float:
        th = _f64(theta)
        if th.size != self._P:
            raise ValueError("theta has the wrong length")
        e = C.c_double()
        self._traj_rows = max(self._traj_rows, 1)
        self._chk(self._lib.vqe_energy(self._h, _p(th, c_f64p), C.byref(e)))
        self._traj_rows = 1
        return e.value

    def energy_batch(self, thetas) -> np.ndarray:
        th = _f64(thetas).reshape(-1, self._P) if self._P else np.zeros((len(thetas), 0))
        out = np.empty(th.shape[0], np.float64)
        self._traj_rows = max(self._traj_rows, th.shape[0])
        self._chk(self._lib.vqe_energy_batch(self._h, th.shape[0], _p(th, c_f64p), _p(out, c_f64p)))
        self._traj_rows = th.shape[0]
        return out

    def energy_grad(self, theta):
        """(E, dE/dtheta) at one parameter vector by the adjoint method on the GPU (n <= 13; n >= 14 after
        set_stream_grad())."""
        th = _f64(theta)
        if th.size != self._P:
            raise ValueError("theta has the wrong length")
        e, g = self.energy_grad_batch(th.reshape(1, -1))
        return float(e[0]), g[0]

    def energy_grad_batch(self, thetas):
        """Energies [B] and gradients [B, P] of the circuit at B parameter vectors (adjoint method)."""
        th = _f64(thetas).reshape(-1, self._P) if self._P else np.zeros((len(thetas), 0))
        e = np.empty(th.shape[0], np.float64)
        g = np.empty((th.shape[0], self._P), np.float64)
        self._chk(self._lib.vqe_energy_grad_batch(self._h, th.shape[0], _p(th, c_f64p), _p(e, c_f64p), _p(g, c_f64p)))
        return e, g

    def get_state(self, theta) -> np.ndarray:
        th = _f64(theta)
        if th.size != self._P:
            raise ValueError("theta has the wrong length")
        out = np.empty(2 << self.n_qubits, np.float64)
        self._chk(self._lib.vqe_get_state(self._h, _p(th, c_f64p), _p(out, c_f64p)))
        return out.view(np.complex128)

    def minimize_cobyla(self, x0, rhobeg=1.0, rhoend=1e-4, maxfun=1000):
        x0 = _f64(x0)
        if x0.size != self._P:
            raise ValueError("x0 has the wrong length")
        x = np.empty_like(x0)
        f = C.c_double()
        nfev = C.c_int32()
        self._chk(self._lib.vqe_minimize_cobyla(self._h, _p(x0, c_f64p), rhobeg, rhoend, int(maxfun),
                                                _p(x, c_f64p), C.byref(f), C.byref(nfev)))
        return x, f.value, nfev.value

    # -- device L-BFGS on the adjoint gradient (NOT scipy's L-BFGS-B: no bounds, Armijo backtracking) ----
    LBFGS_STATUS = {0: "gtol", 1: "ftol", 2: "line search failed", 3: "maxfun", 4: "maxiter"}

    def lbfgs_opts(self, **opts):
        """vqe_lbfgs_opts_t with the library's defaults (history 8, maxiter 100, maxfun 1000, max_ls 20, gtol 1e-6,
        ftol 1e-12, c1 1e-4) and the given fields replaced."""
        o = _lib.LbfgsOpts()
        self._chk(self._lib.vqe_lbfgs_default_opts(C.byref(o)))
        names = {f[0] for f in _lib.LbfgsOpts._fields_}
        for k, v in opts.items():
            if k not in names:
                raise TypeError(f"unknown L-BFGS option {k!r} (known: {sorted(names)})")
            setattr(o, k, float(v) if k in ("gtol", "ftol", "c1") else int(v))
        return o

    def minimize_lbfgs(self, x0, **opts):
        """Minimise E from x0 with the device L-BFGS (one launch).  Returns (x, f, nfev, nit, status)."""
        x0 = _f64(x0)
        if x0.size != self._P:
            raise ValueError("x0 has the wrong length")
        o = self.lbfgs_opts(**opts)
        x = np.empty_like(x0)
        f = C.c_double()
        nfev, nit, st = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._lib.vqe_minimize_lbfgs(self._h, _p(x0, c_f64p), C.byref(o), _p(x, c_f64p), C.byref(f),
                                               C.byref(nfev), C.byref(nit), C.byref(st)))
        return x, f.value, nfev.value, nit.value, st.value

    # -- device Adam-SPSA: two evaluations per iteration, for stochastic energies and many variables ------
    def spsa_opts(self, **opts):
        """vqe_spsa_opts_t with the library's defaults (maxiter 100, a 0.1, alpha 0.602, stability 0, c 0.1, gamma 0.101,
        beta_1 0.9, beta_2 0.999, lamda 0, eps 1e-8, seed 0) and the given fields replaced."""
        o = _lib.SpsaOpts()
        self._chk(self._lib.vqe_spsa_default_opts(C.byref(o)))
        names = {f[0] for f in _lib.SpsaOpts._fields_}
        for k, v in opts.items():
            if k not in names:
                raise TypeError(f"unknown Adam-SPSA option {k!r} (known: {sorted(names)})")
            setattr(o, k, int(v) if k in ("maxiter", "seed") else float(v))
        return o

    def minimize_spsa(self, x0, **opts):
        """Minimise E from x0 with the device Adam-SPSA (one launch, 2 maxiter + 1 evaluations).  Returns (x, f, nfev)."""
        x0 = _f64(x0)
        if x0.size != self._P:
            raise ValueError("x0 has the wrong length")
        o = self.spsa_opts(**opts)
        x = np.empty_like(x0)
        f = C.c_double()
        nfev = C.c_int32()
        self._chk(self._lib.vqe_minimize_spsa(self._h, _p(x0, c_f64p), C.byref(o), _p(x, c_f64p), C.byref(f), C.byref(nfev)))
        return x, f.value, nfev.value

    # -- device Lanczos: extreme eigenpair of the Hamiltonian (no circuit involved) ----------------------
    LANCZOS_STATUS = {0: "converged", 1: "breakdown", 2: "budget"}

    def lanczos_opts(self, which="min", **opts):
        """vqe_lanczos_opts_t with the library's defaults (max_basis 128, max_matvec 2000, check_every 8,
        start_from_init 0, tol 1e-10, seed 1) and the given fields replaced; ``which``: "min" / "max" (or 0 / 1)."""
        o = _lib.LanczosOpts()
        self._chk(self._lib.vqe_lanczos_default_opts(C.byref(o)))
        ends = {"min": 0, "max": 1, 0: 0, 1: 1}
        if which not in ends:
            raise ValueError("which must be 'min' or 'max'")
        o.which = ends[which]
        names = {f[0] for f in _lib.LanczosOpts._fields_} - {"which"}
        for k, v in opts.items():
            if k not in names:
                raise TypeError(f"unknown Lanczos option {k!r} (known: {sorted(names)})")
            setattr(o, k, float(v) if k == "tol" else int(v))
        return o

    def _lanczos_info(self, info):
        return {"residual": info[0], "matvecs": int(info[1]), "restarts": int(info[2]), "status": int(info[3]),
                "status_name": self.LANCZOS_STATUS[int(info[3])]}

    def lanczos(self, which="min", want_vector=True, **opts):
        """The lowest ("min") or highest ("max") eigenvalue of the Hamiltonian and its eigenvector by Lanczos on the
        GPU (vqe_lanczos).  The value is the Rayleigh quotient of the returned vector; it is the extreme pair of the
        Krylov space of the start vector (random by default, the initial state with ``start_from_init=1``).  Returns
        (value, complex128[2^n] or None, info) with info = dict(residual, matvecs, restarts, status, status_name);
        status "budget" is no error - the best pair so far with its true residual."""
        o = self.lanczos_opts(which, **opts)
        ev = C.c_double()
        info = (C.c_double * 4)()
        vec = np.empty(2 << self.n_qubits, np.float64) if want_vector else None
        self._chk(self._lib.vqe_lanczos(self._h, C.byref(o), C.byref(ev), _p(vec, c_f64p) if want_vector else C.cast(None, c_f64p),
                                        info))
        return ev.value, (vec.view(np.complex128) if want_vector else None), self._lanczos_info(info)

    def lanczos_dev(self, dev_ptr: int, which="min", **opts):
        """lanczos with the vector written to device memory (complex128[2^n], asynchronous on the handle's stream; 0: no
        vector).  Returns (value, info)."""
        o = self.lanczos_opts(which, **opts)
        ev = C.c_double()
        info = (C.c_double * 4)()
        self._chk(self._lib.vqe_lanczos_dev(self._h, C.byref(o), C.byref(ev), C.c_void_p(int(dev_ptr) or None), info))
        return ev.value, self._lanczos_info(info)

    def ground_state(self, **opts):
        """(lowest eigenvalue, its eigenvector) of the Hamiltonian by the device Lanczos."""
        value, vec, _ = self.lanczos("min", True, **opts)
        return value, vec

    def lanczos_multi_opts(self, k, which="min", **opts):
        """vqe_lanczos_multi_opts_t with the library's defaults (max_basis 128, max_matvec 2000, check_every 8, keep 0 =
        the library's rule, tol 1e-10, seed 1), ``n_eig = k`` and the given fields replaced."""
        o = _lib.LanczosMultiOpts()
        self._chk(self._lib.vqe_lanczos_multi_default_opts(C.byref(o)))
        ends = {"min": 0, "max": 1, 0: 0, 1: 1}
        if which not in ends:
            raise ValueError("which must be 'min' or 'max'")
        o.which = ends[which]
        o.n_eig = int(k)
        names = {f[0] for f in _lib.LanczosMultiOpts._fields_} - {"which", "n_eig"}
        for key, v in opts.items():
            if key not in names:
                raise TypeError(f"unknown Lanczos option {key!r} (known: {sorted(names)})")
            setattr(o, key, float(v) if key == "tol" else int(v))
        return o

    def _lanczos_multi_info(self, info, res):
        pairs = int(info[4])
        return {"residual": info[0], "matvecs": int(info[1]), "restarts": int(info[2]), "status": int(info[3]),
                "status_name": self.LANCZOS_STATUS[int(info[3])], "pairs": pairs, "residuals": res[:pairs].copy()}

    def lanczos_multi(self, k, which="min", want_vectors=True, **opts):
        """The ``k`` lowest ("min", ascending) or highest ("max", descending) eigenpairs of the Hamiltonian, copies of a
        degenerate eigenvalue included, by thick-restart Lanczos with locking on the GPU (vqe_lanczos_multi).  Returns
        (values[pairs], complex128[pairs, 2^n] or None, info) with info = dict(residual - the largest -, residuals[pairs],
        matvecs, restarts, status, status_name, pairs); pairs = k unless the status is "budget" (no error: the pairs found
        before ``max_matvec`` applications were spent).  ``hamiltonian.level_structure`` groups the values into levels."""
        o = self.lanczos_multi_opts(k, which, **opts)
        k = max(int(k), 1)
        ev, res = np.empty(k, np.float64), np.empty(k, np.float64)
        info = (C.c_double * 5)()
        vec = np.empty((k, 2 << self.n_qubits), np.float64) if want_vectors else None
        self._chk(self._lib.vqe_lanczos_multi(self._h, C.byref(o), _p(ev, c_f64p),
                                              _p(vec, c_f64p) if want_vectors else C.cast(None, c_f64p), _p(res, c_f64p), info))
        d = self._lanczos_multi_info(info, res)
        return ev[:d["pairs"]].copy(), (vec[:d["pairs"]].view(np.complex128) if want_vectors else None), d

    def lanczos_multi_dev(self, dev_ptr: int, k, which="min", **opts):
        """lanczos_multi with the vectors written to device memory (complex128[k, 2^n], asynchronous on the handle's
        stream; 0: no vectors).  Returns (values[pairs], info)."""
        o = self.lanczos_multi_opts(k, which, **opts)
        k = max(int(k), 1)
        ev, res = np.empty(k, np.float64), np.empty(k, np.float64)
        info = (C.c_double * 5)()
        self._chk(self._lib.vqe_lanczos_multi_dev(self._h, C.byref(o), _p(ev, c_f64p), C.c_void_p(int(dev_ptr) or None),
                                                  _p(res, c_f64p), info))
        d = self._lanczos_multi_info(info, res)
        return ev[:d["pairs"]].copy(), d

    # -- batches of circuits --------------------------------------------------------------
    def batch_load(self, circuits, thetas):
        """``circuits``: list of Circuit; ``thetas``: list of arrays (x0 / theta per circuit)."""
        B = len(circuits)
        goff = np.zeros(B + 1, np.int64)
        poff = np.zeros(B + 1, np.int64)
        for b, c in enumerate(circuits):
            goff[b + 1] = goff[b] + len(c)
            poff[b + 1] = poff[b] + c.n_params
        cat = lambda name: (np.concatenate([getattr(c, name) for c in circuits]).astype(np.int32)
                            if goff[-1] else np.zeros(0, np.int32))
        kind, q0, q1, pidx = cat("kind"), cat("q0"), cat("q1"), cat("pidx")
        th = np.concatenate([_f64(t).ravel() for t in thetas]) if poff[-1] else np.zeros(0)
        if th.size != poff[-1]:
            raise ValueError("theta sizes do not match the circuits' parameter counts")
        self.batch_load_flat(goff, kind, q0, q1, pidx, poff, th)

    def batch_load_flat(self, gate_off, kind, q0, q1, pidx, par_off, theta):
        gate_off, par_off = _i64(gate_off), _i64(par_off)
        kind, q0, q1, pidx, theta = _i32(kind), _i32(q0), _i32(q1), _i32(pidx), _f64(theta)
        B = gate_off.size - 1
        self._traj_rows = max(self._traj_rows, B)
        self._chk(self._lib.vqe_batch_load(self._h, B, _p(gate_off, c_i64p), _p(kind, c_i32p), _p(q0, c_i32p),
                                           _p(q1, c_i32p), _p(pidx, c_i32p), _p(par_off, c_i64p), _p(theta, c_f64p)))
        self._batch, self._total_params, self._par_off = B, int(par_off[-1]), par_off
        self._traj_rows = B

    def batch_run_energy(self):
        self._chk(self._lib.vqe_batch_run_energy(self._h))

    def batch_run_reduction(self):
        self._chk(self._lib.vqe_batch_run_reduction(self._h))

    def batch_run_minimize(self, rhobeg=1.0, rhoend=1e-4, maxfun=1000):
        self._chk(self._lib.vqe_batch_run_minimize(self._h, rhobeg, rhoend, int(maxfun)))

    def batch_set_new_gate(self, new_gate):
        if new_gate is None:
            self._chk(self._lib.vqe_batch_set_new_gate(self._h, C.cast(None, c_i32p)))
            return
        ng = _i32(new_gate)
        if ng.size != self._batch:
            raise ValueError("new_gate needs one entry per circuit")
        self._chk(self._lib.vqe_batch_set_new_gate(self._h, _p(ng, c_i32p)))

    def batch_run_env_step(self, rhobeg=1.0, rhoend=1e-4, maxfun=1000):
        self._chk(self._lib.vqe_batch_run_env_step(self._h, rhobeg, rhoend, int(maxfun)))

    def batch_run_minimize_lbfgs(self, **opts):
        """The device L-BFGS on every circuit of the resident batch, one launch (results: batch_fetch, batch_fetch_lbfgs_info)."""
        o = self.lbfgs_opts(**opts)
        self._chk(self._lib.vqe_batch_run_minimize_lbfgs(self._h, C.byref(o)))

    def batch_run_env_step_lbfgs(self, **opts):
        """batch_run_env_step with the device L-BFGS in COBYLA's place (honours batch_set_new_gate)."""
        o = self.lbfgs_opts(**opts)
        self._chk(self._lib.vqe_batch_run_env_step_lbfgs(self._h, C.byref(o)))

    def batch_run_minimize_spsa(self, **opts):
        """The device Adam-SPSA on every circuit of the resident batch, one launch (results: batch_fetch)."""
        o = self.spsa_opts(**opts)
        self._chk(self._lib.vqe_batch_run_minimize_spsa(self._h, C.byref(o)))

    def batch_run_env_step_spsa(self, **opts):
        """batch_run_env_step with the device Adam-SPSA in COBYLA's place (honours batch_set_new_gate)."""
        o = self.spsa_opts(**opts)
        self._chk(self._lib.vqe_batch_run_env_step_spsa(self._h, C.byref(o)))

    def batch_fetch_lbfgs_info(self):
        """(nit, status) per circuit of the last device L-BFGS run."""
        nit = np.empty(self._batch, np.int32)
        st = np.empty(self._batch, np.int32)
        self._chk(self._lib.vqe_batch_fetch_lbfgs_info(self._h, _p(nit, c_i32p), _p(st, c_i32p)))
        return nit, st

    def batch_fetch(self, want_x=True):
        x = np.empty(self._total_params, np.float64) if want_x else None
        f = np.empty(self._batch, np.float64)
        nfev = np.empty(self._batch, np.int32)
        self._chk(self._lib.vqe_batch_fetch(self._h, _p(x, c_f64p) if want_x else C.cast(None, c_f64p),
                                            _p(f, c_f64p), _p(nfev, c_i32p)))
        return x, f, nfev

    def batch_run_energy_grad(self):
        """Energies and gradients of the resident batch (energies: batch_fetch's f, gradients: batch_fetch_grad)."""
        self._chk(self._lib.vqe_batch_run_energy_grad(self._h))

    def batch_fetch_grad(self) -> np.ndarray:
        """Gradients of the last batch_run_energy_grad, concatenated in the layout of batch_fetch's x."""
        g = np.empty(self._total_params, np.float64)
        self._chk(self._lib.vqe_batch_fetch_grad(self._h, _p(g, c_f64p)))
        return g

    def batch_fetch_xopt(self):
        x = np.empty(self._total_params, np.float64)
        self._chk(self._lib.vqe_batch_fetch_xopt(self._h, _p(x, c_f64p)))
        return x

    def batch_energy_devptr(self) -> int:
        p = C.c_void_p()
        self._chk(self._lib.vqe_batch_energy_devptr(self._h, C.byref(p)))
        return int(p.value)

    def batch_copy_energy(self, dst_dev_ptr: int):
        self._chk(self._lib.vqe_batch_copy_energy(self._h, C.c_void_p(int(dst_dev_ptr))))

    def batch_set_trace(self, enable: bool = True):
        self._chk(self._lib.vqe_batch_set_trace(self._h, int(bool(enable))))

    def batch_fetch_trace(self, circuit: int, n_params: int):
        """(f[k], x[k, :n_params]) of every evaluation the device COBYLA loop made for ``circuit``
        in the last traced run (rows beyond its nfev are zero)."""
        mf, st = C.c_int32(), C.c_int32()
        self._chk(self._lib.vqe_batch_fetch_trace(self._h, int(circuit), C.cast(None, c_f64p), C.byref(mf), C.byref(st)))
        out = np.zeros((mf.value, st.value), np.float64)
        self._chk(self._lib.vqe_batch_fetch_trace(self._h, int(circuit), _p(out, c_f64p), C.byref(mf), C.byref(st)))
        return out[:, 0].copy(), out[:, 1:1 + n_params].copy()

    def debug_counters(self):
        out = np.zeros(8, np.uint64)
        self._chk(self._lib.vqe_debug_counters(self._h, _p(out, c_u64p)))
        return out

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._chk(self._lib.vqe_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)


class HostCobyla:
    """ask/tell front end of the library's host COBYLA (same algorithm as the device loop);
    replaces scipy.optimize.minimize(method='COBYLA') where every evaluation needs a
    collective (reference environment_qulacs_TN_notin_agent.py:478)."""

    def __init__(self, x0, rhobeg=1.0, rhoend=1e-4, maxfun=1000):
        self._lib = _lib.load()
        x0 = _f64(x0)
        self.n = int(x0.size)
        self._c = C.c_void_p()
        rc = self._lib.vqe_cobyla_create(self.n, _p(x0, c_f64p), rhobeg, rhoend, int(maxfun), C.byref(self._c))
        if rc:
            raise VQEError(f"vqe_cobyla_create failed ({rc})")
        self._x = np.empty(self.n, np.float64)

    def ask(self):
        rc = self._lib.vqe_cobyla_ask(self._c, _p(self._x, c_f64p))
        if rc < 0:
            raise VQEError("vqe_cobyla_ask failed")
        return self._x.copy() if rc == 1 else None

    def tell(self, f: float):
        rc = self._lib.vqe_cobyla_tell(self._c, float(f))
        if rc < 0:
            raise VQEError("vqe_cobyla_tell failed")

    def result(self):
        x = np.empty(self.n, np.float64)
        f, nfev, st = C.c_double(), C.c_int32(), C.c_int32()
        self._lib.vqe_cobyla_result(self._c, _p(x, c_f64p), C.byref(f), C.byref(nfev), C.byref(st))
        return x, f.value, nfev.value, st.value

    def minimize(self, fun):
        while True:
            x = self.ask()
            if x is None:
                break
            self.tell(fun(x))
        return self.result()

    def __del__(self):
        try:
            if self._c.value:
                self._lib.vqe_cobyla_destroy(self._c)
                self._c = C.c_void_p()
        except Exception:
            pass
