"""B environments stepping in lock-step on one GPU: the MI355X way to reach high
env-steps/s.  Every ``step`` gathers the B post-action circuits and issues ONE fused
launch (COBYLA + float32 round-trip + final energy for all environments).  No reference
counterpart: the reference runs one environment per process (SURVEY.md section 2,
'Parallelism strategies: none').

Two host loops behind the same methods:

* **native** (default where it applies): the bookkeeping of all B environments - gate placement,
  moments, illegal-action slots, the float32 angle commit, rewards, termination, curriculum - runs
  in compiled code (``csrc/vec_env.cpp``, C ABI ``include/vqe_env.h``) on sparse gate lists; the
  observations live in ONE device tensor that every step updates in place (B one-hot writes instead
  of B dense host tensors copied over PCIe).  ``envs[i]`` are read-only views with the attributes the
  reference's driver reads (``nfev, error, energy, prev_energy, rwd, state, moments, opt_ang_save ...``).
* **python**: one ``CircuitEnv`` object per environment (``_core.py``), used for configurations the
  native loop does not cover (curricula other than ``VanillaCurriculum``, ``angles = 1``
  observations) and as the cross-check of the native loop (``tests/test_env_gpu.py``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ._core import CircuitEnvBase
from .utils import curricula

_FIELDS = {"energy": 0, "error": 1, "prev_energy": 2, "nfev": 3, "done_threshold": 4, "step_counter": 5, "rwd": 6,
           "n_gates": 7, "n_rotations": 8, "lowest_energy": 9, "episodes_completed": 10, "halting_step": 11}
# configuration attributes that really are the same for every environment of a batch (read from the prototype); any
# OTHER name is per-environment state the native loop does not expose: an AttributeError, not environment 0's
# construction-time value
_SHARED = frozenset({
    "TN_bond", "TN_init", "TN_state", "_action_index", "_actions_table", "_lmax", "action_size", "cnot_rwd_weight",
    "curriculum_dict", "data_root", "depth_wise_gates", "device", "err_mitig", "fake_min_energy", "fn_type", "geometry",
    "global_iters", "ham", "ham_mapping", "ham_model", "ham_type", "max_eig", "maxfev", "maxfevs", "min_eig", "n_shots",
    "noise_flag", "noise_models", "noise_values", "noisy", "num_layers", "num_layers_termination", "num_qubits", "optim_alg",
    "optim_method", "options", "phys_noise", "random_halt", "spec", "state_size", "state_with_angles", "tn_depth", "tn_gates",
    "weights", "zero_param_init", "engine", "TRAINABLE", "NOISY"})


class _EnvView:
    """Read-only view of environment ``i`` of a native batch."""

    def __init__(self, vec, i):
        self._vec, self._i = vec, i

    def __getattr__(self, name):
        v, i = self._vec, self._i
        if name in _FIELDS:
            val = v._field(name)[i]
            return int(val) if name in ("nfev", "step_counter", "n_gates", "n_rotations", "episodes_completed", "halting_step") else float(val)
        if name == "state":
            return v.state_tensor(i)
        if name == "moments":
            return v._moments(i)[0]
        if name == "illegal_actions":
            return v._moments(i)[1]
        if name == "opt_ang_save":
            return v.opt_ang(i)
        if name == "error_noiseless":
            return float(v._field("error")[i])
        if name in ("current_action", "action", "previous_action"):
            cur, prev = v._actions(i)
            return prev if name == "previous_action" else cur
        if name in _SHARED:
            return getattr(v._proto, name)      # configuration attributes shared by all environments
        raise AttributeError(f"environment view of a native batch has no attribute {name!r} (per-environment state that "
                             "the compiled host loop does not expose; use native=False for the Python objects)")

    def illegal_action_new(self):
        raise RuntimeError("native batch: use VecCircuitEnv.illegal_actions() (one call for all environments)")


class VecCircuitEnv:
    """``device_optimizer``: the optimiser of every step's fused launch, a property of the batch and not of the
    reference's config file - "cobyla" (default: batch_run_env_step, the config's optim_alg = COBYLA) or "lbfgs"
    (batch_run_env_step_lbfgs: the device L-BFGS on adjoint gradients, noiseless configurations and the noisy classes
    with noise_channel = "exact" - set_dm_grad on top of the two switches below; NOT scipy's
    L-BFGS-B; at 14 qubits and more the engine's set_stream_lbfgs is switched on for it).  ``lbfgs_opts``: options of VQEEngine.lbfgs_opts; ``maxfun`` defaults to the config's global_iters so
    that nfev stays comparable with COBYLA's budget.
    "spsa": batch_run_env_step_spsa, the device Adam-SPSA (two evaluations per iteration, energies only): noiseless
    classes, and the noisy classes with noise_channel = "trajectory" and no noise_kraus - depolarising, ``noise_pauli``
    and shot noise; refused with noise_channel = "exact", ``noise_kraus``, ``noise_realisations`` and at 14 qubits and
    more.  ``spsa_opts``: options of VQEEngine.spsa_opts; ``maxiter`` defaults to global_iters // 2, so nfev stays
    within COBYLA's budget.  The reference has no counterpart.
    ``noise_channel``: how the noisy environment classes evaluate their depolarising channels - "trajectory" (default:
    one Pauli trajectory per evaluation, as the reference's qulacs circuits do) or "exact" (the channel those draws
    sample from: the engine's exact channel mode on the batched lock-step path, set_noise_mode(1) + set_dm_batched(-1);
    deterministic energies, 2 <= n <= 13).
    ``noise_kraus``: ``(K1, K2)``, Kraus sets (``channels``) for the channel behind every rotation and behind every CNOT
    in the depolarising channels' place, either of them ``None`` for the depolarising channel; needs
    noise_channel = "exact" (a general channel has no Pauli-trajectory form), or noise_channel = "trajectory" together
    with ``kraus_trajectories`` = T >= 1: every evaluation is then the mean of T quantum-jump trajectories of the
    channel (the engine's set_kraus_traj; at 14 qubits and more the engine's set_stream_kraus_traj is switched on for
    it, while noise_channel = "exact" stays at n <= 13).  Set on the engine once, for the life of the batch.
    ``noise_pauli``: ``(w1, w2)``, Pauli channels for the same two places as probability tables (3 weights of X, Y, Z /
    15 of the two-qubit codes: the engine's set_noise_pauli; ``channels.pauli_weights`` and ``channels.pauli_twirl`` make
    them), either of them ``None`` for the depolarising channel.  Noisy classes only.  With noise_channel = "trajectory"
    the fused sampler draws from the tables (native and Python host loop alike), with "exact" the density matrix runs
    their channel.  A slot takes a table or a Kraus set of ``noise_kraus``, not both.
    ``noise_realisations``: T in [1, 4096]; with device_optimizer = "lbfgs" and noise_channel = "trajectory" on a noisy
    class (with or without ``noise_pauli``) every step's L-BFGS minimises the mean over T frozen Pauli-noise
    realisations of the pre-action circuit (the engine's set_noise_grad) and the step reports ONE fresh trajectory of the
    full circuit, as the COBYLA step does (at 14 qubits and more the engine's set_stream_noise_grad is switched on for
    it).  Without it that combination raises as before."""

    def __init__(self, env_cls, conf, device, num_envs: int, seed: int = 0, native: bool | None = None,
                 device_optimizer: str = "cobyla", lbfgs_opts: dict | None = None, noise_channel: str = "trajectory",
                 noise_kraus=None, kraus_trajectories: int | None = None, noise_pauli=None,
                 noise_realisations: int | None = None, spsa_opts: dict | None = None):
        if not issubclass(env_cls, CircuitEnvBase):
            raise TypeError("env_cls must be one of the CircuitEnv classes of this package")
        if device_optimizer not in ("cobyla", "lbfgs", "spsa"):
            raise ValueError('device_optimizer must be "cobyla", "lbfgs" or "spsa"')
        if spsa_opts is not None and device_optimizer != "spsa":
            raise ValueError('spsa_opts needs device_optimizer = "spsa"')
        if device_optimizer == "spsa":
            if noise_channel == "exact":
                raise NotImplementedError('device_optimizer = "spsa" optimises trajectory energies: noise_channel = "exact" is '
                                          "served by the device COBYLA and the device L-BFGS")
            if noise_kraus is not None:
                raise NotImplementedError('device_optimizer = "spsa" has no quantum-jump form: noise_kraus is served by the '
                                          "device COBYLA")
        if lbfgs_opts is not None and device_optimizer != "lbfgs":
            raise ValueError('lbfgs_opts needs device_optimizer = "lbfgs"')
        if noise_channel not in ("trajectory", "exact"):
            raise ValueError('noise_channel must be "trajectory" or "exact"')
        if noise_channel == "exact" and not getattr(env_cls, "NOISY", False):
            raise ValueError('noise_channel = "exact" is for the noisy environment classes (Pauli noise behind every gate)')
        if kraus_trajectories is not None:
            if noise_kraus is None or noise_channel != "trajectory":
                raise ValueError('kraus_trajectories needs noise_kraus and noise_channel = "trajectory"')
            if not 1 <= int(kraus_trajectories) <= 4096:
                raise ValueError("kraus_trajectories must be in [1, 4096]")
            if not getattr(env_cls, "NOISY", False):
                raise ValueError("kraus_trajectories is for the noisy environment classes (a channel behind every gate)")
        if noise_kraus is not None:
            if noise_channel != "exact" and kraus_trajectories is None:
                raise ValueError('noise_kraus needs noise_channel = "exact"')
            if len(noise_kraus) != 2:
                raise ValueError("noise_kraus is a pair (K1, K2)")
        if noise_pauli is not None:
            if not getattr(env_cls, "NOISY", False):
                raise ValueError("noise_pauli is for the noisy environment classes (a channel behind every gate)")
            if len(noise_pauli) != 2:
                raise ValueError("noise_pauli is a pair (w1, w2)")
            if noise_kraus is not None and any(w is not None and K is not None for w, K in zip(noise_pauli, noise_kraus)):
                raise ValueError("a noise slot takes a Pauli table (noise_pauli) or a Kraus set (noise_kraus), not both")
        if noise_realisations is not None:
            if device_optimizer != "lbfgs" or noise_channel != "trajectory" or noise_kraus is not None:
                raise ValueError('noise_realisations needs device_optimizer = "lbfgs" and noise_channel = "trajectory" '
                                 "(Pauli channels: depolarising or noise_pauli)")
            if not getattr(env_cls, "NOISY", False):
                raise ValueError("noise_realisations is for the noisy environment classes (a channel behind every gate)")
            if not 1 <= int(noise_realisations) <= 4096:
                raise ValueError("noise_realisations must be in [1, 4096]")
        first = env_cls(conf, device, seed=seed)
        if first.optimizer_kind not in (None, "device_cobyla"):
            raise NotImplementedError(f"VecCircuitEnv runs the device COBYLA of batch_run_env_step only; optim_alg = "
                                      f"{first.optim_alg!r} is served by CircuitEnv")
        self.device_optimizer = device_optimizer
        self._lbfgs_opts = None
        self._spsa_opts = None
        if device_optimizer == "spsa":
            if first.num_qubits >= 14:
                raise NotImplementedError('device_optimizer = "spsa" runs for n_qubits <= 13 (the LDS-resident path) only')
            self._spsa_opts = {"maxiter": int(first.global_iters) // 2, **(spsa_opts or {})}
            first.engine.spsa_opts(**self._spsa_opts)      # (unknown names raise here, not at the first step)
        if device_optimizer == "lbfgs":
            frozen = noise_realisations is not None and not first.n_shots
            if noise_channel != "exact" and (first.NOISY or first.phys_noise or first.n_shots) and not frozen:
                raise NotImplementedError("device_optimizer = 'lbfgs' needs an exact, deterministic energy: noisy and "
                                          "finite-shot configurations are served by the device COBYLA, or by "
                                          "noise_channel = 'exact' (the channel itself, a density matrix), or - Pauli "
                                          "noise without shot noise - on frozen draws (noise_realisations = T)")
            self._lbfgs_opts = {"maxfun": int(first.global_iters), **(lbfgs_opts or {})}
        self.engine = first.engine
        self.noise_channel = noise_channel
        if noise_channel == "exact":
            self.engine.set_noise_mode(1)
            self.engine.set_dm_batched(-1)
            if device_optimizer == "lbfgs":
                self.engine.set_dm_grad(True)            # the adjoint gradient of tr(rho H) on the batched path
            if noise_kraus is not None:                  # (after the constructor's set_noise and its get_state)
                self.engine.set_noise_kraus(noise_kraus[0], noise_kraus[1])
        if kraus_trajectories is not None:               # (after the constructor's set_noise and its get_state)
            if device_optimizer != "cobyla":
                raise NotImplementedError("quantum-jump trajectories are served by the device COBYLA")
            self.engine.set_noise_kraus(noise_kraus[0], noise_kraus[1])
            self.engine.set_kraus_traj(int(kraus_trajectories))
            if first.num_qubits >= 14:
                self.engine.set_stream_kraus_traj(-1)    # the streaming path runs trajectories on request only
        if noise_pauli is not None:                      # (after the constructor's set_noise, which leaves tables alone)
            self.engine.set_noise_pauli(noise_pauli[0], noise_pauli[1])
        if noise_realisations is not None:               # (the counter stays where the constructor's runs left it)
            self.engine.set_noise_grad(int(noise_realisations))
            if first.num_qubits >= 14:
                self.engine.set_stream_noise_grad(-1)    # the streaming path runs the noisy gradients on request only
        if device_optimizer == "lbfgs" and first.num_qubits >= 14:
            self.engine.set_stream_lbfgs(True)           # the streaming path runs the device L-BFGS on request only
        self._proto = first
        self.num_envs = num_envs
        self.device = device
        self.num_qubits, self.num_layers = first.num_qubits, first.num_layers
        self.state_size, self.action_size = first.state_size, first.action_size
        self._pending = None
        supported = (isinstance(first.curriculum_dict[first.ham_type], curricula.VanillaCurriculum)
                     and not first.state_with_angles and first.fn_type == "incremental_with_fixed_ends"
                     and first.optim_method == "scipy_each_step")
        if native is None:
            native = supported
        if native and not supported:
            raise ValueError("the native host loop covers VanillaCurriculum, angles = 0, scipy_each_step configurations")
        self.native = bool(native)
        if self.native:
            self._init_native(first, conf)
        else:
            self.envs = [first] + [env_cls(conf, device, engine=self.engine) for _ in range(num_envs - 1)]
            for e in self.envs[1:]:
                e.TN_state = first.TN_state

    # ---- native batch ------------------------------------------------------------------------
    def _init_native(self, first, conf):
        lib = _lib.load()
        self._lib = lib
        n, L, B = self.num_qubits, self.num_layers, self.num_envs
        self.engine._traj_rows = B          # the compiled loop loads its batches itself (engine.batch_fetch_traj)
        base_obs = first.reset()                         # E(initial circuit), TN encoding of the trainable path
        st = first.state.numpy()
        lay, row, col = np.nonzero(st[:, :n + 3, :] == 1)
        kind = np.where(row < n, 0, row - n + 1).astype(np.int32)
        q0 = col.astype(np.int32)                        # CNOT: [target][control]; rotation: [axis][qubit]
        q1 = np.where(row < n, row, -1).astype(np.int32)
        ang = np.where(row < n, 0.0, st[lay, np.minimum(row + 3, n + 5), col]).astype(np.float32)
        cur = first.curriculum_dict[first.ham_type]
        thr = np.ascontiguousarray(cur.thresholds, np.float64)
        swe = np.ascontiguousarray(cur.episodes, np.int64)
        table = np.ascontiguousarray([first._actions_table[i] for i in range(len(first._actions_table))], np.int32)
        self._keep = (thr, swe, table, lay.astype(np.int32), kind, q0, q1, ang)       # arrays the config points to
        p32 = lambda a: a.ctypes.data_as(_lib.c_i32p)
        cfg = _lib.VecEnvConfig(
            n_qubits=n, num_layers=L, num_envs=B, layer_offset=first._tn_offset(), noisy=int(first.NOISY),
            num_layers_termination=int(first.num_layers_termination), maxfun=int(first.global_iters),
            min_eig=float(first.min_eig), accept_err=float(conf["env"]["accept_err"]),
            n_thresholds=int(thr.size), thresholds=thr.ctypes.data_as(_lib.c_f64p), switch_episodes=swe.ctypes.data_as(_lib.c_i64p),
            n_init_gates=int(kind.size), init_layer=p32(self._keep[3]), init_kind=p32(kind), init_q0=p32(q0), init_q1=p32(q1),
            init_angle=ang.ctypes.data_as(C.POINTER(C.c_float)), init_energy=float(first.prev_energy),
            n_actions=int(table.shape[0]), action_table=p32(table))
        self._h = C.c_void_p()
        rc = lib.vqe_vecenv_create(C.byref(cfg), self.engine._h, C.byref(self._h))
        if rc:
            raise _lib.VQEError(f"vqe_vecenv_create failed ({rc})")
        if self._lbfgs_opts is not None:
            o = self.engine.lbfgs_opts(**self._lbfgs_opts)
            self._chk(lib.vqe_vecenv_set_optimizer(self._h, 1, C.byref(o)))
        if self._spsa_opts is not None:
            o = self.engine.spsa_opts(**self._spsa_opts)
            self._chk(lib.vqe_vecenv_set_optimizer_spsa(self._h, C.byref(o)))
        self._base_obs = base_obs.to(self.device)
        self._obs = self._base_obs.repeat(B, 1)
        self._cache = {}
        self.envs = [_EnvView(self, i) for i in range(B)]
        self._random_halt = bool(first.random_halt)

    def _chk(self, rc):
        if rc:
            msg = self._lib.vqe_vecenv_last_error(self._h)
            raise _lib.VQEError(f"native environment batch error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "native", False) and getattr(self, "_h", None) is not None and self._h.value:
            self._lib.vqe_vecenv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _field(self, name):
        a = self._cache.get(name)
        if a is None:
            a = np.empty(self.num_envs, np.float64)
            self._chk(self._lib.vqe_vecenv_get(self._h, _FIELDS[name], a.ctypes.data_as(_lib.c_f64p)))
            self._cache[name] = a
        return a

    def _moments(self, i):
        n = self.num_qubits
        m = np.empty(n, np.int32)
        s = np.empty((n, 4), np.int32)
        self._chk(self._lib.vqe_vecenv_moments(self._h, int(i), m.ctypes.data_as(_lib.c_i32p), s.ctypes.data_as(_lib.c_i32p)))
        return [int(v) for v in m], [[int(v) for v in r] if r[0] >= 0 else [] for r in s]

    def _actions(self, i):
        cur, prev = np.zeros(4, np.int32), np.zeros(4, np.int32)
        self._chk(self._lib.vqe_vecenv_actions(self._h, int(i), cur.ctypes.data_as(_lib.c_i32p), prev.ctypes.data_as(_lib.c_i32p)))
        return [int(x) for x in cur], [int(x) for x in prev]

    def state_tensor(self, i):
        """Dense (L, n+6, n) float32 state tensor of environment ``i`` (what ``CircuitEnv.state`` holds)."""
        n, L = self.num_qubits, self.num_layers
        out = np.empty((L, n + 6, n), np.float32)
        self._chk(self._lib.vqe_vecenv_state(self._h, int(i), out.ctypes.data_as(C.POINTER(C.c_float))))
        return torch.from_numpy(out)

    def opt_ang(self, i):
        cnt = C.c_int32()
        self._chk(self._lib.vqe_vecenv_opt_ang(self._h, int(i), C.cast(None, _lib.c_f64p), C.byref(cnt)))
        out = np.empty(cnt.value, np.float64)
        if cnt.value:
            self._chk(self._lib.vqe_vecenv_opt_ang(self._h, int(i), out.ctypes.data_as(_lib.c_f64p), C.byref(cnt)))
        return out

    @property
    def nfev(self):
        return self._field("nfev") if self.native else np.array([e.nfev for e in self.envs], np.float64)

    @property
    def errors(self):
        return self._field("error") if self.native else np.array([e.error for e in self.envs], np.float64)

    def last_kernel_ms(self):
        return self.engine.last_kernel_ms()

    # ---- API ---------------------------------------------------------------------------------
    def reset(self, indices=None):
        if not self.native:
            idx = range(self.num_envs) if indices is None else indices
            return torch.stack([self.envs[i].reset() for i in idx])
        self._cache = {}
        idx = None if indices is None else np.ascontiguousarray(list(indices), np.int32)
        cnt = self.num_envs if idx is None else int(idx.size)
        halt = None
        if self._random_halt:      # rand_halt configs draw the halting step per episode (reference reset() :350-352)
            halt = np.clip(np.random.negative_binomial(n=70, p=0.573, size=cnt), 25, 70).astype(np.int32)
        self._chk(self._lib.vqe_vecenv_reset(
            self._h, cnt, idx.ctypes.data_as(_lib.c_i32p) if idx is not None else C.cast(None, _lib.c_i32p),
            halt.ctypes.data_as(_lib.c_i32p) if halt is not None else C.cast(None, _lib.c_i32p)))
        if idx is None:
            self._obs = self._base_obs.repeat(self.num_envs, 1)
            return self._obs.clone()
        rows = torch.as_tensor(idx.astype(np.int64), device=self.device)
        self._obs[rows] = self._base_obs
        return self._obs[rows].clone()

    def illegal_actions_array(self):
        """(B, n) int32, action indices in ascending order, -1 padded (native batch only)."""
        out = np.empty((self.num_envs, self.num_qubits), np.int32)
        self._chk(self._lib.vqe_vecenv_illegal_actions(self._h, out.ctypes.data_as(_lib.c_i32p)))
        return out

    def illegal_actions(self):
        if not self.native:
            return [e.illegal_action_new() for e in self.envs]
        return [[int(a) for a in row if a >= 0] for row in self.illegal_actions_array()]

    def step_async(self, actions):
        """First half of ``step``: host bookkeeping before the optimiser and the (asynchronous)
        fused launch.  The caller may do unrelated host work - typically ``step_wait`` +
        action selection of ANOTHER VecCircuitEnv (each has its own engine and HIP stream) -
        before collecting the results with ``step_wait``."""
        if self._pending is not None:
            raise RuntimeError("step_async called twice without step_wait")
        if self.native:
            a = np.ascontiguousarray(actions, np.int32).reshape(self.num_envs, 4)
            self._chk(self._lib.vqe_vecenv_step_begin(self._h, a.ctypes.data_as(_lib.c_i32p)))
            self._pending = (None, a)
            return
        pre = [e._pre_step(a) for e, a in zip(self.envs, actions)]
        eng = self.engine
        eng.batch_load([p[1] for p in pre], [p[2] for p in pre])
        eng.batch_set_new_gate([p[3] for p in pre])
        if self._lbfgs_opts is not None:
            eng.batch_run_env_step_lbfgs(**self._lbfgs_opts)
        elif self._spsa_opts is not None:
            eng.batch_run_env_step_spsa(**self._spsa_opts)
        else:
            eng.batch_run_env_step(1.0, 1e-4, int(self.envs[0].global_iters))
        self._pending = (pre, actions)

    def step_wait(self, train_flag=True):
        """Second half of ``step``: wait for the launch, commit angles / rewards / termination.
        Returns (observations (B, obs), rewards (B,), dones list[int])."""
        if self._pending is None:
            raise RuntimeError("step_wait without step_async")
        pre, actions = self._pending
        self._pending = None
        if self.native:
            B = self.num_envs
            rwd = np.empty(B, np.float32)
            done = np.empty(B, np.int32)
            oix = np.empty(B, np.int64)
            self._chk(self._lib.vqe_vecenv_step_end(self._h, int(bool(train_flag)), rwd.ctypes.data_as(C.POINTER(C.c_float)),
                                                    done.ctypes.data_as(_lib.c_i32p), oix.ctypes.data_as(_lib.c_i64p)))
            self._cache = {}
            rows = np.nonzero(oix >= 0)[0]
            if rows.size:      # the observation tensor lives on the device: one one-hot write per environment
                self._obs[torch.as_tensor(rows, device=self.device), torch.as_tensor(oix[rows], device=self.device)] = 1.0
            return self._obs.clone(), torch.from_numpy(rwd).to(self.device), [int(d) for d in done]
        eng = self.engine
        x, f, nfev = eng.batch_fetch()
        xo = eng.batch_fetch_xopt()
        obs, rwd, done = [], [], []
        off = 0
        for b, (e, p, a) in enumerate(zip(self.envs, pre, actions)):
            P = p[1].n_params
            o, r, d = e._post_step(p[0], p[1], x[off:off + P], e._strip_new(p[1], p[3], xo[off:off + P]), float(f[b]), int(nfev[b]), a,
                                   train_flag, to_device=False)
            off += P
            obs.append(o), rwd.append(r), done.append(d)
        # one host-to-device copy for the whole batch
        return (torch.stack(obs).to(self.device),
                torch.tensor(rwd, dtype=torch.float32).to(self.device), done)

    def step(self, actions, train_flag=True):
        """``actions``: B lists [ctrl, offset, rot_qubit, rot_axis].  Returns
        (observations (B, obs), rewards (B,), dones list[int])."""
        self.step_async(actions)
        return self.step_wait(train_flag)
