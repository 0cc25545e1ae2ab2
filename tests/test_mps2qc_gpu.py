"""GPU parity of the MPS -> PQC fit (libmps2qc_hip.so, through its C ABI) against the numpy
restatement of dmrg-to-qc/stiefel_opt.py + mps2qc.py (oracle/stiefel_oracle.py).

Tolerances: environments / overlaps of one step <= 1e-12, gates after one update <= 1e-12, loss
histories over 60 steps <= 1e-10, gates after 60 steps <= 1e-9 (rounding differences of the
FMA-contracted device arithmetic grow slowly along the trajectory)."""
import numpy as np
import pytest

import stiefel_oracle as so
from helpers import MPS2QC_OUTPUTS, load_case, mps2qc_raw_fit, oracle_init_state

pytestmark = pytest.mark.gpu


def _problem(n, layers, rng, batch=2, representable=True):
    from tensorrl_qas_amd import dmrg_to_qc as dq
    sites, G = dq.brickwork_ansatz(n, layers)
    assert list(sites) == so.brickwork_pairs(n, layers)
    if representable:
        tg = [so.circuit_state(n, sites, so.random_unitaries(G, rng)) for _ in range(batch)]
    else:
        tg = []
        for _ in range(batch):
            v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
            tg.append(v / np.linalg.norm(v))
    init = np.array([so.random_unitaries(G, rng) for _ in range(batch)])
    return sites, G, np.array(tg), init


@pytest.mark.parametrize("mfma", [True, False])
@pytest.mark.parametrize("n,layers", [(2, 1), (3, 2), (4, 1), (5, 2), (6, 1), (7, 3), (8, 1), (9, 2), (10, 1),
                                      (11, 2), (12, 1), (12, 4)])
def test_one_step_matches_oracle(n, layers, mfma):
    from tensorrl_qas_amd import dmrg_to_qc as dq
    rng = np.random.default_rng(100 * n + layers)
    sites, G, tg, init = _problem(n, layers, rng, representable=(n % 2 == 0))
    for frozen in (False, True):
        opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=frozen, use_mfma=mfma)
        opt.init(init)
        opt.minimize(dq.BrickworkOverlap(n, sites, tg), init, max_iter=1, tol=1e-30, param_tol=0.0)
        for b in range(len(init)):
            o, envs = so.overlap_and_envs(n, list(sites), list(init[b]), tg[b])
            assert abs(opt.last_overlap[b] - o) < 1e-12
            assert np.max(np.abs(opt.last_envs[b] - np.array(envs))) < 1e-12
            ref = so.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=frozen)
            ref.init(init[b])
            bv, bp, hist, fin = ref.minimize(n, list(sites), tg[b], init[b], max_iter=1, tol=1e-30, param_tol=0.0)
            assert np.max(np.abs(opt.final_params[b] - np.array(fin))) < 1e-12
            assert np.max(np.abs(opt.opt_params[b] - np.array(bp))) < 1e-12
            assert abs(opt.best_val[b] - bv) < 1e-12 and opt.n_iter[b] == 1
            assert abs(opt.loss_history[b][0] - hist[0]) < 1e-12


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("n,layers", [(4, 2), (6, 1), (9, 1), (12, 1)])
def test_trajectory_matches_oracle(n, layers, frozen):
    from tensorrl_qas_amd import dmrg_to_qc as dq
    rng = np.random.default_rng(7 * n + layers)
    sites, G, tg, init = _problem(n, layers, rng, batch=2)
    steps = 60 if n < 12 else 25
    opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=frozen)
    opt.init(init)
    opt.minimize(dq.BrickworkOverlap(n, sites, tg), init, max_iter=steps, tol=1e-12, param_tol=1e-9)
    for b in range(2):
        ref = so.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=frozen)
        ref.init(init[b])
        bv, bp, hist, fin = ref.minimize(n, list(sites), tg[b], init[b], max_iter=steps, tol=1e-12, param_tol=1e-9)
        assert opt.n_iter[b] == len(hist)
        assert np.max(np.abs(np.array(opt.loss_history[b]) - np.array(hist))) < 1e-10
        assert np.max(np.abs(opt.final_params[b] - np.array(fin))) < 1e-9
        assert np.max(np.abs(opt.opt_params[b] - np.array(bp))) < 1e-9
        assert abs(opt.best_val[b] - bv) < 1e-10
        for g in opt.final_params[b]:
            assert np.max(np.abs(g @ g.conj().T - np.eye(4))) < 1e-12
        assert hist[-1] < hist[0]


def test_large_learning_rate_and_termination():
    """A big step (lr = 0.3: I - a/2 far from the identity, complex velocities after the
    transport) and both stopping rules of minimize()."""
    from tensorrl_qas_amd import dmrg_to_qc as dq
    rng = np.random.default_rng(5)
    n, layers = 5, 2
    sites, G, tg, init = _problem(n, layers, rng, batch=3)
    opt = dq.StiefelAdam(0.3, 0.9, 0.99, 1e-10)
    opt.init(init)
    opt.minimize(dq.BrickworkOverlap(n, sites, tg), init, max_iter=8, tol=1e-12, param_tol=1e-9)
    for b in range(3):
        ref = so.StiefelAdam(0.3, 0.9, 0.99, 1e-10)
        ref.init(init[b])
        bv, bp, hist, fin = ref.minimize(n, list(sites), tg[b], init[b], max_iter=8, tol=1e-12, param_tol=1e-9)
        assert np.max(np.abs(np.array(opt.loss_history[b]) - np.array(hist))) < 1e-9
        assert np.max(np.abs(opt.final_params[b] - np.array(fin))) < 1e-8
    # tol: start at the exact solution -> loss ~ 1e-16 < tol after one step
    exact = np.array([so.random_unitaries(G, rng)])
    t = so.circuit_state(n, sites, exact[0])
    opt.minimize(dq.BrickworkOverlap(n, sites, t), exact, max_iter=50, tol=1e-8, param_tol=0.0)
    assert opt.n_iter[0] == 1 and opt.best_val[0] < 1e-12
    # param_tol: with a vanishing learning rate the gates do not move
    opt2 = dq.StiefelAdam(1e-12, 0.9, 0.999, 1e-8)
    opt2.minimize(dq.BrickworkOverlap(n, sites, tg), init, max_iter=50, tol=1e-30, param_tol=1e-6)
    assert list(opt2.n_iter) == [1, 1, 1]


def test_shared_target_many_restarts_fit_golden_init_state():
    """End to end: the reference's shipped H2O-8q init circuit (21 cx + 129 rotations = 7 SU(4)
    blocks, one brickwork layer) is exactly representable; 64 restarts fitted in one launch."""
    from tensorrl_qas_amd import dmrg_to_qc as dq
    psi = oracle_init_state(load_case("H2O_8q"))
    n = 8
    rng = np.random.default_rng(0)
    opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=True)
    gates, hist, params = dq.mps_to_qc(psi, {"structure": "brickwork", "num_layers": 1},
                                       {"method": opt, "max_iter": 3000, "tol": 1e-8}, n_restarts=64, rng=rng)
    sites, G = dq.brickwork_ansatz(n, 1)
    assert G == 7 and len(gates) == 7
    best = float(np.min(opt.best_val))
    assert best < 5e-3, best
    # the loss the kernel reports is the loss of the gates one step earlier; the returned
    # gates are at least as good up to one step of size lr
    assert so.loss(n, list(sites), gates, psi) < best + 1e-2
    assert hist[-1] <= hist[0]
    assert all(np.max(np.abs(g @ g.conj().T - np.eye(4))) < 1e-10 for g in gates)


def test_mfma_and_valu_agree_and_errors():
    from tensorrl_qas_amd import dmrg_to_qc as dq, VQEError
    rng = np.random.default_rng(11)
    n, layers = 10, 2
    sites, G, tg, init = _problem(n, layers, rng, batch=4, representable=False)
    res = []
    for mfma in (True, False):
        opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, use_mfma=mfma)
        opt.minimize(dq.BrickworkOverlap(n, sites, tg), init, max_iter=40, tol=1e-12, param_tol=1e-9)
        res.append((np.array(opt.loss_history), opt.final_params.copy()))
    assert np.max(np.abs(res[0][0] - res[1][0])) < 1e-11
    assert np.max(np.abs(res[0][1] - res[1][1])) < 1e-10
    with pytest.raises(VQEError):   # 13 qubits do not fit the LDS-resident kernel (by default they take the streaming one)
        dq.StiefelAdam(stream=False).minimize(dq.BrickworkOverlap(13, np.zeros(1, np.int32), np.zeros(1 << 13, complex)),
                                              np.eye(4)[None, None], max_iter=1)
    s12, G12 = dq.brickwork_ansatz(12, 6)  # 66 gates do not fit beside two 64-KiB states
    with pytest.raises(VQEError):
        dq.StiefelAdam().minimize(dq.BrickworkOverlap(12, s12, np.ones(1 << 12, complex) / 64),
                                  np.tile(np.eye(4), (1, G12, 1, 1)), max_iter=1)


def test_fit_to_qasm_to_engine_state(tmp_path):
    """The offline pipeline end to end: fit on the GPU -> {rz, ry, cx} text -> the reader and the
    state-vector engine the environments use.  The engine's state equals the brickwork state of
    the fitted gates (register qubit k = MPS site k), and its overlap with the target is the one
    the fit reports."""
    import tensorrl_qas_amd as tq
    from tensorrl_qas_amd import dmrg_to_qc as dq
    psi_t = oracle_init_state(load_case("BEH2_6q"))          # little-endian target from the shipped circuit
    n = 6
    rev = np.array([int(format(i, f"0{n}b")[::-1], 2) for i in range(1 << n)])
    target = psi_t[rev]                                       # site 0 most significant
    rng = np.random.default_rng(3)
    opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=True)
    gates, hist, _ = dq.mps_to_qc(target, {"structure": "brickwork", "num_layers": 1},
                                  {"method": opt, "max_iter": 1500, "tol": 1e-8}, n_restarts=32, rng=rng)
    sites, G = dq.brickwork_ansatz(n, 1)
    path = tmp_path / "init_BEH2_6q_TNbond2.qasm"
    dq.mps2qc.write_init_circuit(path, n, sites, gates, rng)
    nq, parsed = tq.qasm.parse(open(path).read())
    circ, ang = tq.circuits.circuit_from_qasm_gates(parsed)
    eng = tq.VQEEngine(n, 0)
    eng.set_circuit(circ)
    state = eng.get_state(ang)
    ref = so.circuit_state(n, list(sites), gates)
    assert abs(abs(np.vdot(ref[rev], state)) - 1) < 1e-9
    assert abs((1 - abs(np.vdot(psi_t, state))) - so.loss(n, list(sites), gates, target)) < 1e-9
    assert 1 - abs(np.vdot(psi_t, state)) < np.min(opt.best_val) + 1e-2


@pytest.mark.parametrize("n", [6, 12])
def test_arbitrary_gate_sequences(n):
    """Gate lists that are not brickwork: a staircase (every run of disjoint gates has one gate),
    a single gate, and runs whose paired gates are far apart / in descending order."""
    from tensorrl_qas_amd import dmrg_to_qc as dq
    rng = np.random.default_rng(n)
    for sites in ([0, 1, 2, 3, 4], [n - 2], [n - 2, 0, 2, 1, n - 3, 0], [0, n - 2, 2, 1, 3, 0]):
        sites = np.array(sites, np.int32)
        G = len(sites)
        v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
        tg = v / np.linalg.norm(v)
        init = np.array([so.random_unitaries(G, rng) for _ in range(2)])
        opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8)
        opt.minimize(dq.BrickworkOverlap(n, sites, tg), init, max_iter=3, tol=1e-30, param_tol=0.0)
        for b in range(2):
            ref = so.StiefelAdam(3e-3, 0.9, 0.999, 1e-8)
            ref.init(init[b])
            bv, bp, hist, fin = ref.minimize(n, list(sites), tg, init[b], max_iter=3, tol=1e-30, param_tol=0.0)
            assert np.max(np.abs(np.array(opt.loss_history[b]) - np.array(hist))) < 1e-12
            assert np.max(np.abs(opt.final_params[b] - np.array(fin))) < 1e-11
            o, envs = so.overlap_and_envs(n, list(sites), list(fin_prev(ref, n, sites, tg, init[b])), tg)
            assert np.max(np.abs(opt.last_envs[b] - np.array(envs))) < 1e-11


def fin_prev(ref, n, sites, tg, init):
    """Gates before the last of 3 steps (the environments the kernel reports belong to them)."""
    r2 = so.StiefelAdam(ref.learning_rate, ref.beta1, ref.beta2, ref.eps)
    r2.init(init)
    return r2.minimize(n, list(sites), tg, init, max_iter=2, tol=1e-30, param_tol=0.0)[3]


# ---- HBM-streaming variant (registers beyond 12 qubits) ------------------------------------------
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("n,layers,steps", [(6, 2, 30), (12, 1, 15), (13, 1, 12), (14, 2, 8), (16, 1, 4)])
def test_streaming_fit_matches_oracle(n, layers, steps, frozen):
    """mps2qc_fit_brickwork_stream (states in HBM, fused backward sweep + environment reduction per gate,
    Stiefel update on the host) against the numpy restatement: overlap / environments of the last step,
    loss history, final and best gates - the tolerances of the LDS-resident kernel; 13 .. 16 qubits are
    beyond MPS2QC_MAX_QUBITS, the small sizes tie the two kernels to the same oracle."""
    from tensorrl_qas_amd import dmrg_to_qc as dq
    rng = np.random.default_rng(31 * n + layers)
    sites, G, tg, init = _problem(n, layers, rng, batch=2, representable=(n <= 13))
    opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=frozen, stream=True)
    opt.init(init)
    opt.minimize(dq.BrickworkOverlap(n, sites, tg), init, max_iter=steps, tol=1e-12, param_tol=1e-9)
    for b in range(2):
        ref = so.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=frozen)
        ref.init(init[b])
        bv, bp, hist, fin = ref.minimize(n, list(sites), tg[b], init[b], max_iter=steps, tol=1e-12, param_tol=1e-9)
        assert opt.n_iter[b] == len(hist)
        assert np.max(np.abs(np.array(opt.loss_history[b]) - np.array(hist))) < 1e-10
        assert np.max(np.abs(opt.final_params[b] - np.array(fin))) < 1e-9
        assert np.max(np.abs(opt.opt_params[b] - np.array(bp))) < 1e-9
        assert abs(opt.best_val[b] - bv) < 1e-10
        for g in opt.final_params[b]:
            assert np.max(np.abs(g @ g.conj().T - np.eye(4))) < 1e-12


def test_streaming_fit_equals_lds_kernel_and_defaults_by_size():
    """Same problem through both kernels (n = 10): loss histories and gates agree to rounding; StiefelAdam picks
    the streaming kernel by itself beyond 12 qubits; a 20-qubit fit (16 MiB states) runs and descends."""
    from tensorrl_qas_amd import dmrg_to_qc as dq
    rng = np.random.default_rng(5)
    sites, G, tg, init = _problem(10, 2, rng, batch=3)
    runs = []
    for stream in (False, True):
        opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, stream=stream)
        opt.init(init)
        opt.minimize(dq.BrickworkOverlap(10, sites, tg), init, max_iter=40, tol=1e-12, param_tol=1e-9)
        runs.append(opt)
    for b in range(3):
        assert np.max(np.abs(np.array(runs[0].loss_history[b]) - np.array(runs[1].loss_history[b]))) < 1e-11
        assert np.max(np.abs(runs[0].final_params[b] - runs[1].final_params[b])) < 1e-10
    n = 20
    sites, G = dq.brickwork_ansatz(n, 1)
    tgt = so.circuit_state(n, list(sites), so.random_unitaries(G, rng))
    start = np.array([so.random_unitaries(G, rng)])
    opt = dq.StiefelAdam(3e-2, 0.9, 0.999, 1e-8)                       # stream=None: by size
    opt.init(start)
    opt.minimize(dq.BrickworkOverlap(n, sites, tgt), start, max_iter=12, tol=1e-12, param_tol=0.0)
    h = opt.loss_history[0]
    assert len(h) == 12 and h[-1] < h[0] and 0.0 < h[-1] <= 1.0
    o = np.vdot(tgt, so.circuit_state(n, list(sites), list(start[0])))
    assert abs(h[0] - (1.0 - abs(o))) < 1e-10
    with pytest.raises(Exception):
        dq.StiefelAdam(3e-3, stream=False).minimize(dq.BrickworkOverlap(n, sites, tgt), start, max_iter=1)    # LDS kernel: n <= 12


def test_ground_state_to_init_circuit_to_environment(tmp_path):
    """The offline chain the reference runs with DMRG + quimb + qiskit (dmrg-to-qc/dmrg_to_qc.py:137-223), here for
    a 14-qubit Heisenberg chain beyond the LDS-resident fit: generator -> Lanczos ground state -> streaming
    brickwork fit -> {rz, ry, cx} text -> CircuitEnv.  The environment's initial energy is the energy of the
    fitted circuit: far below the synthetic stand-in, above the ground energy, and consistent with the
    reported fidelity (E - E0 <= (1 - F^2) (E_max - E0))."""
    import torch
    import tensorrl_qas_amd as tq
    from tensorrl_qas_amd import synthetic
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    n = 14
    conf = synthetic.write_chain_dataset(str(tmp_path / "fit"), n, init="fit",
                                         fit_opts={"max_iter": 400, "n_restarts": 4, "num_layers": 2})
    env = CircuitEnv(conf, torch.device("cuda:0"))
    env.reset()
    ham, _ = tq.hamiltonian.heisenberg(n)
    e0, psi = tq.hamiltonian.ground_state(ham)
    assert abs(env.min_eig - e0) < 1e-8
    fid = abs(np.vdot(psi, env.TN_state))
    e_fit = float(env.prev_energy)
    conf2 = synthetic.write_chain_dataset(str(tmp_path / "syn"), n, eigvals=[e0, 2 * n - 1.0])
    env2 = CircuitEnv(conf2, torch.device("cuda:0"))
    env2.reset()
    assert e0 - 1e-9 <= e_fit < float(env2.prev_energy) - 1.0          # a fitted start beats a random one by a lot
    assert fid > 0.5
    assert e_fit - e0 <= (1.0 - fid ** 2) * (env.max_eig - e0) + 1e-9


# ---- the host layer, through the raw C ABI ---------------------------------------------------------
def _raw_problem(n, layers, seed):
    rng = np.random.default_rng(seed)
    sites = so.brickwork_pairs(n, layers)
    tg = np.array([so.circuit_state(n, sites, so.random_unitaries(len(sites), rng)) for _ in range(2)])
    init = np.array([so.random_unitaries(len(sites), rng) for _ in range(2)])
    return sites, tg, init


_ORACLE4 = {}


def _assert_valid_fit4(stream):
    """A valid 4-qubit fit (2 layers, batch 2, 3 steps) returns 0, matches the oracle and clears the message."""
    from tensorrl_qas_amd import _lib
    sites, tg, init = _raw_problem(4, 2, 404)
    if not _ORACLE4:
        for b in range(2):
            ref = so.StiefelAdam(3e-3, 0.9, 0.999, 1e-8)
            ref.init(init[b])
            _ORACLE4[b] = ref.minimize(4, list(sites), tg[b], init[b], max_iter=3, tol=1e-30, param_tol=0.0)
    rc, out = mps2qc_raw_fit(stream, 4, sites, tg, init, 3)
    assert rc == 0 and _lib.load_mps2qc().mps2qc_last_error() == b""
    for b in range(2):
        bv, bp, hist, fin = _ORACLE4[b]
        assert out["n_iter"][b] == 3 and abs(out["best_val"][b] - bv) < 1e-12
        assert np.max(np.abs(out["loss_history"][b] - np.array(hist))) < 1e-12
        assert np.max(np.abs(out["final_gates"][b] - np.array(fin))) < 1e-11
        assert np.max(np.abs(out["opt_gates"][b] - np.array(bp))) < 1e-11


@pytest.mark.parametrize("stream", [False, True])
def test_null_outputs_through_the_c_abi(stream):
    """Every output pointer NULL except best_val: the call returns 0 and best_val is, bit for bit, that of the call
    with all outputs."""
    sites, tg, init = _raw_problem(4, 2, 404)
    rc_all, full = mps2qc_raw_fit(stream, 4, sites, tg, init, 3)
    rc_one, one = mps2qc_raw_fit(stream, 4, sites, tg, init, 3, only=("best_val",))
    assert rc_all == 0 and rc_one == 0
    assert list(one) == ["best_val"] and one["best_val"].tobytes() == full["best_val"].tobytes()
    assert np.all(full["best_val"] > 0) and np.all(full["n_iter"] == 3)


def test_error_then_success_on_one_thread():
    """A refused layout (12 qubits, 66 gates) and a gate outside the register leave a message and no debris: the
    valid fit that follows on the same thread matches the oracle and mps2qc_last_error() is empty again."""
    from tensorrl_qas_amd import _lib
    lib = _lib.load_mps2qc()
    s12 = so.brickwork_pairs(12, 6)
    flat = np.ones(1 << 12, complex) / 64
    rc, _ = mps2qc_raw_fit(False, 12, s12, flat, np.tile(np.eye(4), (1, len(s12), 1, 1)), 1)
    assert len(s12) == 66 and rc == -22 and b"LDS" in lib.mps2qc_last_error()
    _assert_valid_fit4(False)
    sites, tg, init = _raw_problem(4, 2, 404)
    for stream in (False, True):
        bad = np.array(sites, np.int32)
        bad[3] = 3      # the pair (3, 4) of a 4-qubit register
        rc, _ = mps2qc_raw_fit(stream, 4, bad, tg, init, 3)
        assert rc == -22 and b"gate 3 on sites (3,4) outside the register" in lib.mps2qc_last_error()
        _assert_valid_fit4(stream)


def test_stream_graph_replay_equals_plain_launches(tmp_path):
    """MPS2QC_STREAM_GRAPH is read once per process: two fresh interpreters (tests/rank_workers.py), one with the
    knob at 0, run the same streaming fit; every output is bit-identical."""
    from rank_workers import run_ranks
    res = []
    for knob in ("1", "0"):
        d = tmp_path / f"graph{knob}"
        d.mkdir()
        res.append(run_ranks("mps2qc_stream_fit", 1, d, timeout=120, extra_env={"MPS2QC_STREAM_GRAPH": knob})[0])
    assert res[0]["rc"] == 0 and res[1]["rc"] == 0
    assert set(res[0]) == {"rc", *MPS2QC_OUTPUTS} and res[0] == res[1]
    assert np.all(np.frombuffer(bytes.fromhex(res[0]["n_iter"]), np.int32) == 5)


def test_alternating_paths_in_one_process():
    """LDS fit, streaming fit, LDS fit at 6 qubits: the first and the third are bit-identical."""
    sites, tg, init = _raw_problem(6, 2, 606)
    runs = [mps2qc_raw_fit(stream, 6, sites, tg, init, 5) for stream in (False, True, False)]
    assert [rc for rc, _ in runs] == [0, 0, 0]
    for k in MPS2QC_OUTPUTS:
        assert runs[0][1][k].tobytes() == runs[2][1][k].tobytes(), k
