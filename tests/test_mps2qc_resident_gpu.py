"""GPU: the resident streaming fit (mps2qc_fit_brickwork_resident, StiefelAdam(update="device"): sweeps through HBM,
Stiefel-Adam update and the bookkeeping of minimize() on the device) against the numpy restatement
(oracle/stiefel_oracle.py) and against the host-update streaming fit.  Optimiser 3e-3, 0.9, 0.999, 1e-8 throughout.

Tolerances.  Against the oracle those of test_streaming_fit_matches_oracle: n_iter equal, histories and best_val
<= 1e-10, gates <= 1e-9, unitarity <= 1e-12; overlap and environments of the last executed step <= 1e-11
(test_arbitrary_gate_sequences).  Against the host-update path twice the first two: both paths are within 1e-10 / 1e-9
of the oracle, so 2e-10 / 2e-9 is the most two correct paths can differ."""
import numpy as np
import pytest

import stiefel_oracle as so
from mps2qc_resident_helpers import OPTIMISER, bit_reversed, resident_raw_fit, same_bits

pytestmark = pytest.mark.gpu

TOL, PARAM_TOL = 1e-12, 1e-9

# n, layers, steps, batch, shared target: the smallest shapes at which each part can still go wrong
SHAPES = {
    "n2_one_vector": (2, 1, 20, 2, False),           # one 4-vector in the whole state, G = 1
    "n3": (3, 2, 20, 2, False),
    "n10_one_block": (10, 2, 15, 2, False),          # exactly one block of 4-vectors
    "n11_two_blocks": (11, 1, 12, 2, False),         # the first real second-stage reduction
    "n14_many_blocks": (14, 2, 8, 2, False),         # beyond the LDS kernel
    "n6_G70": (6, 14, 6, 2, False),                  # more gates than a wavefront's four, no multiple of 16
    "n4_G270": (4, 90, 4, 2, False),                 # several passes of the gate loop in one workgroup
    "n5_batch1": (5, 2, 10, 1, False),
    "n5_batch3_shared": (5, 2, 10, 3, True),
}

_PROBLEMS, _ORACLE = {}, {}


def _problem(name):
    """sites, targets ([batch][2^n], or [2^n] when shared), start gates: drawn once per shape, never changed"""
    if name not in _PROBLEMS:
        n, layers, steps, batch, shared = SHAPES[name]
        rng = np.random.default_rng(1000 + sorted(SHAPES).index(name))
        sites = so.brickwork_pairs(n, layers)
        G = len(sites)
        if n <= 13:
            tg = [so.circuit_state(n, sites, so.random_unitaries(G, rng)) for _ in range(1 if shared else batch)]
        else:
            tg = []
            for _ in range(batch):
                v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
                tg.append(v / np.linalg.norm(v))
        tg = np.array(tg[0] if shared else tg)
        init = np.array([so.random_unitaries(G, rng) for _ in range(batch)])
        for a in (tg, init):
            a.setflags(write=False)
        _PROBLEMS[name] = (sites, tg, init)
    return _PROBLEMS[name]


def _oracle(name, frozen):
    """Per fit: (best_val, best gates, history, final gates, overlap and environments at the gates before the last
    update).  Computed once and shared."""
    key = (name, frozen)
    if key not in _ORACLE:
        n, layers, steps, batch, shared = SHAPES[name]
        sites, tg, init = _problem(name)
        res = []
        for b in range(batch):
            t = tg if shared else tg[b]
            ref = so.StiefelAdam(*OPTIMISER, jit_frozen=frozen)
            ref.init(init[b])
            bv, bp, hist, fin = ref.minimize(n, list(sites), t, init[b], max_iter=steps, tol=TOL, param_tol=PARAM_TOL)
            prev = [np.array(g) for g in init[b]]
            if len(hist) > 1:
                r2 = so.StiefelAdam(*OPTIMISER, jit_frozen=frozen)
                r2.init(init[b])
                prev = r2.minimize(n, list(sites), t, init[b], max_iter=len(hist) - 1, tol=0.0, param_tol=-1.0)[3]
            o, envs = so.overlap_and_envs(n, list(sites), list(prev), t)
            res.append((bv, np.array(bp), np.array(hist), np.array(fin), o, np.array(envs)))
        _ORACLE[key] = res
    return _ORACLE[key]


def _device(name, frozen, update="device"):
    from tensorrl_qas_amd import dmrg_to_qc as dq
    n, layers, steps, batch, shared = SHAPES[name]
    sites, tg, init = _problem(name)
    opt = dq.StiefelAdam(*OPTIMISER, jit_frozen=frozen, stream=True, update=update)
    opt.init(init)
    opt.minimize(dq.BrickworkOverlap(n, np.array(sites, np.int32), tg), init, max_iter=steps, tol=TOL, param_tol=PARAM_TOL)
    return opt


# ---- (a) against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_resident_fit_matches_oracle(name, frozen):
    n, layers, steps, batch, shared = SHAPES[name]
    opt = _device(name, frozen)
    assert opt.steps_enqueued is not None and opt.steps_enqueued >= max(opt.n_iter)
    for b, (bv, bp, hist, fin, o, envs) in enumerate(_oracle(name, frozen)):
        figures = (np.max(np.abs(np.array(opt.loss_history[b]) - hist)) if opt.n_iter[b] == len(hist) else None,
                   np.max(np.abs(opt.final_params[b] - fin)), np.max(np.abs(opt.opt_params[b] - bp)),
                   abs(opt.last_overlap[b] - o), np.max(np.abs(opt.last_envs[b] - envs)))
        print(name, frozen, b, "n_iter", opt.n_iter[b], "hist / final / best / overlap / envs:", figures)
        assert opt.n_iter[b] == len(hist)
        assert figures[0] <= 1e-10
        assert abs(opt.best_val[b] - bv) <= 1e-10
        assert figures[1] <= 1e-9 and figures[2] <= 1e-9
        for g in opt.final_params[b]:
            assert np.max(np.abs(g @ g.conj().T - np.eye(4))) <= 1e-12
        assert figures[3] <= 1e-11 and figures[4] <= 1e-11


# ---- (b) against the host-update path -----------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("name", ["n10_one_block", "n14_many_blocks"])
def test_resident_fit_matches_host_update(name, frozen):
    dev, host = _device(name, frozen), _device(name, frozen, update="host")
    assert host.steps_enqueued is None
    assert list(dev.n_iter) == list(host.n_iter)
    dh = max(np.max(np.abs(np.array(a) - np.array(b))) for a, b in zip(dev.loss_history, host.loss_history))
    dg = max(np.max(np.abs(dev.final_params - host.final_params)), np.max(np.abs(dev.opt_params - host.opt_params)))
    print(name, frozen, "device against host update: histories", dh, "gates", dg)
    assert dh <= 2e-10 and dg <= 2e-9


# ---- (c) lock-step and termination ---------------------------------------------------------------------------------
def _lockstep_problem():
    n, rng = 6, np.random.default_rng(66)
    sites = so.brickwork_pairs(n, 1)
    G = len(sites)
    exact = so.random_unitaries(G, rng)
    tg = np.array([so.circuit_state(n, sites, exact), so.circuit_state(n, sites, so.random_unitaries(G, rng))])
    init = np.array([exact, so.random_unitaries(G, rng)])      # fit 0 starts at the gates that generate its target
    return n, sites, tg, init


def test_lockstep_termination_and_check_every():
    from tensorrl_qas_amd import _lib
    n, sites, tg, init = _lockstep_problem()
    runs = {}
    for ce, want in ((1, 10), (4, 12), (16, 16)):
        rc, out, enq = resident_raw_fit(n, sites, tg, init, 10, tol=1e-12, opts={"check_every": ce})
        assert rc == 0, _lib.load_mps2qc().mps2qc_last_error()
        assert enq == want
        runs[ce] = out
    same_bits(runs[1], runs[4])
    same_bits(runs[1], runs[16])
    out = runs[1]
    assert list(out["n_iter"]) == [1, 10]
    assert np.all(out["loss_history"][0, 1:] == 0.0) and out["loss_history"][0, 0] < 1e-12
    assert np.all(out["loss_history"][1] > 0.0)
    # the host-update path with the same stopping rule (tol = 1e-12, param_tol = 0) through the Python layer
    from tensorrl_qas_amd import dmrg_to_qc as dq
    host = dq.StiefelAdam(*OPTIMISER, stream=True)
    host.minimize(dq.BrickworkOverlap(n, np.array(sites, np.int32), tg), init, max_iter=10, tol=1e-12, param_tol=0.0)
    assert list(host.n_iter) == [1, 10]
    figures = (np.max(np.abs(out["final_gates"][0] - host.final_params[0])), np.max(np.abs(out["last_envs"][0] - host.last_envs[0])),
               abs(out["last_overlap"][0] - host.last_overlap[0]))
    print("stopped fit against the host update: final gates / last_envs / last_overlap", figures)
    assert figures[0] <= 2e-9 and figures[1] <= 2e-9 and figures[2] <= 2e-10
    assert np.max(np.abs(out["loss_history"][1] - np.array(host.loss_history[1]))) <= 2e-10
    assert np.max(np.abs(out["final_gates"][1] - host.final_params[1])) <= 2e-9


# ---- (d) targets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_target_sources_and_orders(shared):
    import torch
    n, rng = 5, np.random.default_rng(55 + shared)      # odd: the bit reversal is no palindrome of the index bits
    sites = so.brickwork_pairs(n, 2)
    G = len(sites)
    tg = np.array([so.circuit_state(n, sites, so.random_unitaries(G, rng)) for _ in range(2)])
    tg = tg[0] if shared else tg
    init = np.array([so.random_unitaries(G, rng) for _ in range(2)])
    rev = bit_reversed(n)
    assert not np.array_equal(rev, np.arange(1 << n)) and np.array_equal(rev[rev], np.arange(1 << n))
    le = np.ascontiguousarray(tg[..., rev])              # the same state(s) in the engine's order
    assert not np.array_equal(le, tg)
    dev = lambda a: torch.from_numpy(a).to("cuda:0")
    rc, ref, _ = resident_raw_fit(n, sites, tg, init, 6)
    assert rc == 0 and np.all(ref["n_iter"] == 6)
    for target, opts in ((dev(tg), {"target_on_device": 1}),
                         (le, {"target_little_endian": 1}),
                         (dev(le), {"target_on_device": 1, "target_little_endian": 1})):
        rc, out, _ = resident_raw_fit(n, sites, target, init, 6, opts=opts)
        assert rc == 0
        same_bits(ref, out)
    # and through the Python layer: a tensor target takes the device update by itself
    from tensorrl_qas_amd import dmrg_to_qc as dq
    opt = dq.StiefelAdam(*OPTIMISER)
    opt.minimize(dq.BrickworkOverlap(n, np.array(sites, np.int32), dev(le), "little_endian"), init, max_iter=6, tol=1e-30,
                 param_tol=0.0)
    assert opt.steps_enqueued == 8 and opt.final_params.tobytes() == ref["final_gates"].tobytes()
    with pytest.raises(ValueError):
        opt.minimize(dq.BrickworkOverlap(n, np.array(sites, np.int32), dev(le).to(torch.complex64)), init, max_iter=1)
    with pytest.raises(ValueError):
        dq.StiefelAdam(*OPTIMISER, stream=False, update="device").minimize(
            dq.BrickworkOverlap(n, np.array(sites, np.int32), tg), init, max_iter=1)


# ---- (e) graph on and off ----------------------------------------------------------------------------------------------
def _problem6():
    rng = np.random.default_rng(606)
    sites = so.brickwork_pairs(6, 2)
    tg = np.array([so.circuit_state(6, sites, so.random_unitaries(len(sites), rng)) for _ in range(2)])
    init = np.array([so.random_unitaries(len(sites), rng) for _ in range(2)])
    return sites, tg, init


def test_graph_replay_equals_plain_launches():
    sites, tg, init = _problem6()
    rc0, plain, _ = resident_raw_fit(6, sites, tg, init, 5, opts={"use_graph": 0})
    rc1, graph, _ = resident_raw_fit(6, sites, tg, init, 5, opts={"use_graph": 1})
    assert rc0 == 0 and rc1 == 0 and np.all(plain["n_iter"] == 5)
    same_bits(plain, graph)


# ---- (f) the ABI ---------------------------------------------------------------------------------------------------------
_ORACLE4 = {}


def _assert_valid_fit4():
    """A valid 4-qubit fit (2 layers, batch 2, 3 steps) returns 0, matches the oracle and clears the message."""
    from tensorrl_qas_amd import _lib
    rng = np.random.default_rng(404)
    sites = so.brickwork_pairs(4, 2)
    tg = np.array([so.circuit_state(4, sites, so.random_unitaries(len(sites), rng)) for _ in range(2)])
    init = np.array([so.random_unitaries(len(sites), rng) for _ in range(2)])
    if not _ORACLE4:
        for b in range(2):
            ref = so.StiefelAdam(*OPTIMISER)
            ref.init(init[b])
            _ORACLE4[b] = ref.minimize(4, list(sites), tg[b], init[b], max_iter=3, tol=1e-30, param_tol=0.0)
    rc, out, enq = resident_raw_fit(4, sites, tg, init, 3)
    assert rc == 0 and _lib.load_mps2qc().mps2qc_last_error() == b"" and enq == 8
    for b in range(2):
        bv, bp, hist, fin = _ORACLE4[b]
        assert out["n_iter"][b] == 3 and abs(out["best_val"][b] - bv) < 1e-12
        assert np.max(np.abs(out["loss_history"][b] - np.array(hist))) < 1e-12
        assert np.max(np.abs(out["final_gates"][b] - np.array(fin))) < 1e-11
        assert np.max(np.abs(out["opt_gates"][b] - np.array(bp))) < 1e-11
    return sites, tg, init


def test_null_opts_are_the_defaults_and_single_outputs():
    import ctypes as C
    from tensorrl_qas_amd import _lib
    lib = _lib.load_mps2qc()
    o = _lib.ResidentOpts()
    assert lib.mps2qc_resident_default_opts(C.byref(o)) == 0
    assert (o.target_on_device, o.target_little_endian, o.check_every, o.use_graph) == (0, 0, 8, -1)
    assert lib.mps2qc_resident_default_opts(None) == -22
    sites, tg, init = _problem6()
    rc_null, null, enq_null = resident_raw_fit(6, sites, tg, init, 5, opts=None)
    rc_def, dflt, enq_def = resident_raw_fit(6, sites, tg, init, 5, opts={})
    assert rc_null == 0 and rc_def == 0 and enq_null == enq_def == 8
    same_bits(null, dflt)
    for k in null:      # one requested output only, every other pointer NULL
        rc, one, _ = resident_raw_fit(6, sites, tg, init, 5, only=(k,))
        assert rc == 0 and list(one) == [k] and one[k].tobytes() == null[k].tobytes(), k


def test_refusals_then_success_on_one_thread():
    from tensorrl_qas_amd import _lib
    lib = _lib.load_mps2qc()
    sites, tg, init = _assert_valid_fit4()
    bad_sites = np.array(sites, np.int32)
    bad_sites[3] = 3      # the pair (3, 4) of a 4-qubit register
    refusals = [dict(opts={"check_every": 0}), dict(opts={"check_every": -3}),
                dict(opts={"target_on_device": 2}), dict(opts={"target_on_device": -1}),
                dict(opts={"target_little_endian": 2}), dict(opts={"use_graph": 2}), dict(opts={"use_graph": -2}),
                dict(opts={"target_on_device": 1}),              # a host pointer called device memory
                dict(sites=bad_sites), dict(steps=0), dict(n=27)]      # what begin_fit refuses
    for r in refusals:
        rc, out, enq = resident_raw_fit(r.get("n", 4), r.get("sites", sites), tg, init, r.get("steps", 3), opts=r.get("opts"))
        assert rc == -22 and lib.mps2qc_last_error() != b"", r
        assert enq == -1 and all(not v.any() for v in out.values()), r      # nothing was launched or written
        _assert_valid_fit4()


def test_alternating_with_the_host_update_path():
    """Resident fit, host-update streaming fit, resident fit at 6 qubits: the first and the third are the same bits."""
    from helpers import mps2qc_raw_fit
    sites, tg, init = _problem6()
    first = resident_raw_fit(6, sites, tg, init, 5)
    rc, host = mps2qc_raw_fit(True, 6, sites, tg, init, 5)
    third = resident_raw_fit(6, sites, tg, init, 5)
    assert first[0] == 0 and rc == 0 and third[0] == 0
    same_bits(first[1], third[1])
    assert np.max(np.abs(first[1]["loss_history"] - host["loss_history"])) <= 2e-10
    assert np.max(np.abs(first[1]["final_gates"] - host["final_gates"])) <= 2e-9


# ---- (g) the chain --------------------------------------------------------------------------------------------------------
def test_chain_ground_state_to_fit_without_the_host_hop():
    """13-qubit Heisenberg: device Lanczos -> fit with the state never leaving the device, against the same chain
    through host memory with the same seed.  The optimisers are handed in (with the hyperparameters
    fit_state_to_init_circuit would choose) only because that is where the loss histories can be read."""
    import torch
    import tensorrl_qas_amd as tq
    from tensorrl_qas_amd import dmrg_to_qc as dq
    from tensorrl_qas_amd.dmrg_to_qc.mps2qc import fit_state_to_init_circuit
    n = 13
    ham, _ = tq.hamiltonian.heisenberg(n)
    e_dev, vec = tq.hamiltonian.ground_state_device(ham, return_tensor=True)
    assert isinstance(vec, torch.Tensor) and vec.is_cuda and vec.dtype == torch.complex128 and vec.shape == (1 << n,)
    opt_dev = dq.StiefelAdam(3e-2, 0.9, 0.999, 1e-8)
    text, infid, gates, sites = fit_state_to_init_circuit(vec, num_layers=1, max_iter=60, n_restarts=1,
                                                          rng=np.random.default_rng(6), optimizer=opt_dev)
    assert opt_dev.steps_enqueued is not None
    e_host, psi = tq.hamiltonian.ground_state_device(ham)
    opt_host = dq.StiefelAdam(3e-2, 0.9, 0.999, 1e-8)
    text_h, infid_h, gates_h, _ = fit_state_to_init_circuit(psi, num_layers=1, max_iter=60, n_restarts=1,
                                                            rng=np.random.default_rng(6), optimizer=opt_host)
    assert opt_host.steps_enqueued is None and abs(e_dev - e_host) < 1e-9
    hd, hh = np.array(opt_dev.loss_history[0][:20]), np.array(opt_host.loss_history[0][:20])
    print("chain: histories of the first 20 steps differ by", np.max(np.abs(hd - hh)), "n_iter", opt_dev.n_iter, opt_host.n_iter)
    assert len(hd) == 20 and len(hh) == 20 and np.max(np.abs(hd - hh)) <= 2e-10
    # the same state from host memory with update="device": no numpy reversal, the same bits as from the tensor
    _, infid_n, gates_n, _ = fit_state_to_init_circuit(psi, num_layers=1, max_iter=60, n_restarts=1, rng=np.random.default_rng(6),
                                                       update="device")
    if vec.cpu().numpy().tobytes() == psi.tobytes():      # the two Lanczos runs returned the same vector
        assert infid_n == infid and np.array(gates_n).tobytes() == np.array(gates).tobytes()
    assert abs(infid_n - infid) <= 2e-10
    # The reported infidelity is, by the bookkeeping of minimize(), the loss of the gates BEFORE the update of the best
    # step, the returned gates are those AFTER it (observed at 60 steps: 0.21840 reported, 0.21678 for the returned
    # gates - one step of size lr apart), so the two are not comparable at 1e-9.  What is: the reported value is the
    # lowest entry of the history, and the loss the device reports FOR the returned gates - the first loss of a fit
    # started from them on the same device tensor - equals the oracle's.
    assert infid == min(opt_dev.loss_history[0]) == opt_dev.best_val[0]
    again = dq.StiefelAdam(3e-2, 0.9, 0.999, 1e-8)
    again.minimize(dq.BrickworkOverlap(n, np.array(sites, np.int32), vec, "little_endian"), np.array(gates)[None], max_iter=1,
                   tol=1e-30, param_tol=0.0)
    gs = vec.cpu().numpy()[bit_reversed(n)]              # site 0 most significant, the oracle's order
    direct = so.loss(n, list(sites), gates, gs)
    print("chain: oracle infidelity of the returned gates", direct, "device", again.loss_history[0][0], "reported best", infid)
    assert abs(direct - again.loss_history[0][0]) <= 1e-9
    assert direct < infid + 1e-2                         # at least as good up to one step of size lr
