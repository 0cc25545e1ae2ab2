"""GPU: the device Adam-SPSA (k_lds_minimize_spsa; vqe_minimize_spsa, vqe_batch_run_minimize_spsa,
vqe_batch_run_env_step_spsa) against its numpy restatement (tests/spsa_helpers.py) and the CPU oracle.

The main test is teacher-forced: every energy of a device trace must equal the oracle's energy at the recorded point
with the same evaluation id within 1e-10 Ha, and the restatement fed the device's own f+ / f- values must reproduce every
recorded trial point, xraw and xopt within 1e-12 max(1, |x|) - the rounding of a dozen operations per element and
iteration; no decision of the algorithm can amplify it.  tests/test_spsa_cpu.py checks the preconditions and the
sensitivities of the free-run cases on the CPU."""
import numpy as np
import pytest

import lbfgs_helpers as lh
import noise_pauli_oracle as npo
import spsa_helpers as sh
import vqe_oracle as vo
from helpers import random_gates, random_hamiltonian, random_state, rotations, with_noise_gates

pytestmark = pytest.mark.gpu

E_TOL = 1e-10         # energies: the project's 1e-10 Ha
X_TOL = 1e-12         # teacher-forced points, times max(1, |x|)
ESTATE, EINVAL = -1, -22


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _engine(tq, n, ham, psi0):
    eng = tq.VQEEngine(n, 0)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    return eng


def _close(got, want, tol=X_TOL):
    got, want = np.asarray(got), np.asarray(want)
    dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    return float(dev.max(initial=0.0)) <= tol, float(dev.max(initial=0.0))


def _pre_action(gates, theta, new_gate, noisy):
    """-> (gates of the circuit the optimiser sees, hole).  A noisy list has a noise gate behind every gate: the new
    gate leaves with its own.  The parameter indices above the hole move down (the oracle takes compact angles)."""
    kind, q0, q1, pidx = gates
    if new_gate < 0:
        return gates, -1
    hole = int(pidx[new_gate])
    keep = np.ones(kind.size, bool)
    keep[new_gate] = False
    if noisy:
        keep[new_gate + 1] = False
    p2 = pidx[keep].copy()
    if hole >= 0:
        p2[p2 > hole] -= 1
    return (kind[keep], q0[keep], q1[keep], p2), hole


def _energy(psi0, gates, x, ham, noise, b, eid):
    """The oracle's mode 0 energy with evaluation id eid at position b"""
    case = dict(psi0=psi0, gates=gates, ham=ham)
    return sh.oracle_objective(case, eval_base=eid, b=b, noise=noise)(np.asarray(x, np.float64), 0)


def _check_teacher_forced(eng, b, psi0, ham, gates, theta, new_gate, env, opts, x, xopt, f, nfev, noise=None, eval_base=0):
    """Circuit b of a traced run against the oracle and the restatement; returns the worst point deviation."""
    P = theta.size
    noisy = noise is not None and (4 in gates[0] or 5 in gates[0])
    pre, hole = _pre_action(gates, theta, new_gate if env else -1, noisy)
    Popt = P - (hole >= 0)
    K = int(opts["maxiter"]) if Popt > 0 else 0
    tf, tx = eng.batch_fetch_trace(b, P)
    rows = 2 * K if (env and K > 0) else 2 * K + 1
    assert np.all(tf[rows:] == 0.0) and np.all(tx[rows:] == 0.0)
    pts = sh.unpack_trace(tx, P, hole)
    keep = [j for j in range(P) if j != hole]
    worst_e = 0.0
    for e in range(2 * K):
        ref = _energy(psi0, pre, pts[e][keep], ham, noise, b, eval_base + e)
        print(f"circuit {b} evaluation {e}: device {tf[e]:.12f} oracle {ref:.12f} |dE| {abs(tf[e] - ref):.2e}")
        worst_e = max(worst_e, abs(tf[e] - ref))
        assert abs(tf[e] - ref) <= E_TOL, (b, e, tf[e], ref)
    r = sh.spsa(None, theta, hole=hole, b=b, feed=list(tf[:2 * K]), **opts)
    worst = 0.0
    for e in range(2 * K):
        ok, dev = _close(pts[e][keep], r.trials[e][keep])
        worst = max(worst, dev)
        assert ok, (b, e, dev)
    ok, dev = _close(xopt, r.x)
    worst = max(worst, dev)
    print(f"circuit {b}: K = {K}, worst point deviation {worst:.2e}, worst |dE| {worst_e:.2e}")
    assert ok, (b, "xopt", dev)
    if hole >= 0:
        assert xopt[hole] == theta[hole]
    if env:
        assert np.array_equal(x, xopt.astype(np.float32).astype(np.float64))
        assert nfev == (2 * K if K > 0 else 1)
        if K == 0:      # the closing evaluation alone, and it has the trace row
            assert tf[0] == f
    else:
        assert np.array_equal(x, xopt) and nfev == 2 * K + 1
        assert np.array_equal(pts[2 * K][keep], xopt[keep]) and tf[2 * K] == f      # the final f of a plain run in row 2K
    ref = _energy(psi0, gates, x, ham, noise, b, eval_base + 2 * K)
    assert abs(f - ref) <= E_TOL, (b, "closing", f, ref)
    return worst


def _run(tq, eng, circuits, opts, new_gates=None, env=False, noise=None, eval_base=0, psi0=None, ham=None):
    """Load, run traced, check every circuit teacher-forced.  circuits: [(gates, theta)]"""
    eng.batch_load([tq.Circuit(*g, th.size) for g, th in circuits], [th for _, th in circuits])
    if new_gates is not None:
        eng.batch_set_new_gate(new_gates)
    eng.batch_set_trace(True)
    (eng.batch_run_env_step_spsa if env else eng.batch_run_minimize_spsa)(**opts)
    x, f, nfev = eng.batch_fetch()
    xopt = eng.batch_fetch_xopt()
    off = 0
    for b, (g, th) in enumerate(circuits):
        P = th.size
        _check_teacher_forced(eng, b, psi0, ham, g, th, new_gates[b] if new_gates is not None else -1, env, opts,
                              x[off:off + P], xopt[off:off + P], float(f[b]), int(nfev[b]), noise, eval_base)
        off += P
    eng.batch_set_trace(False)
    return x, f, nfev


# ---- teacher-forced parity -------------------------------------------------------------------------------------------------
# (n, K, su4): 5 the LDS path below kRegMinQubits, 9 / 10 / 12 the register path in both WIDE geometries, 13
PARITY = [(1, 8, False), (5, 8, False), (6, 6, True), (9, 6, False), (10, 6, False), (12, 6, False), (12, 6, True), (13, 4, False)]


@pytest.mark.parametrize("n,K,su4", PARITY, ids=[f"n{n}-K{K}-{'su4' if s else 'rot'}" for n, K, s in PARITY])
def test_teacher_forced_parity(tq, n, K, su4):
    case = lh.trajectory_case(n, 0, su4)
    eng = _engine(tq, n, case["ham"], case["psi0"])
    opts = dict(maxiter=K, seed=100 + n)
    _run(tq, eng, [(case["gates"], case["theta"])], opts, psi0=case["psi0"], ham=case["ham"])
    eng.close()


def test_teacher_forced_130_parameters(tq):
    """n = 8, P = 130: several strides of the element loop (64 threads); plain run and an env-step with a hole"""
    n, P = 8, 130
    rng = np.random.default_rng(88)
    g = rotations(n, P, rng)
    gates, theta = g[:4], g[4]
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 24, rng, real=False)
    eng = _engine(tq, n, ham, psi0)
    opts = dict(maxiter=4, seed=5)
    _run(tq, eng, [(gates, theta)], opts, psi0=psi0, ham=ham)
    ng = int(np.nonzero(gates[0] != 0)[0][70])
    _run(tq, eng, [(gates, theta)], opts, new_gates=[ng], env=True, psi0=psi0, ham=ham)
    eng.close()


# ---- free run --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sh.FREE_CASES, ids=lambda k: f"n{k[0]}-h{k[1]}")
def test_free_run_against_the_restatement_on_oracle_energies(tq, key):
    """Default options, seed 7, K = 30: all 61 points within 10 x the case's CPU-measured sensitivity (the deviation of
    the restatement's points under N(0, 1e-10) energies), computed in the helper from the restatement alone."""
    case = sh.free_case(*key)
    ref, sens = sh.free_run(*key)
    tol = 10.0 * sens
    eng = _engine(tq, case["n"], case["ham"], case["psi0"])
    eng.batch_load([tq.Circuit(*case["gates"], case["theta"].size)], [case["theta"]])
    eng.batch_set_trace(True)
    eng.batch_run_minimize_spsa(**sh.FREE_OPTS)
    x, f, nfev = eng.batch_fetch()
    tf, tx = eng.batch_fetch_trace(0, case["theta"].size)
    eng.batch_set_trace(False)
    assert nfev[0] == ref.nfev == 61
    worst = max(float(np.abs(tx[e] - ref.trials[e]).max()) for e in range(61))
    print(f"{key}: tolerance {tol:.2e} (sensitivity {sens:.2e}), observed deviation {worst:.2e}")
    assert worst <= tol
    assert np.abs(x - ref.x).max() <= tol and abs(f[0] - ref.f) <= E_TOL + tol * case["scale"]
    start = lh.oracle_energy(case["psi0"], *case["gates"], case["theta"], case["ham"])
    assert f[0] < start
    eng.close()


# ---- noise -----------------------------------------------------------------------------------------------------------------
NOISE_SEED = 424242


def _noise_setting(eng, kind):
    w1, w2 = npo.TABLES["distinct"]
    if kind == "depol":
        eng.set_noise(0.01, 0.05, NOISE_SEED)
        return dict(seed=NOISE_SEED, p1=0.01, p2=0.05, shot_seed=NOISE_SEED)
    if kind == "pauli":
        eng.set_noise(0.0, 0.0, NOISE_SEED)
        eng.set_noise_pauli(w1, w2)
        return dict(seed=NOISE_SEED, w1=w1, w2=w2, shot_seed=NOISE_SEED)
    eng.set_noise(0.01, 0.05, NOISE_SEED)      # "shot": the shot term on top of depolarising draws (one seed for both)
    eng.set_shot_noise(0.05, NOISE_SEED)
    return dict(seed=NOISE_SEED, p1=0.01, p2=0.05, shot_sigma=0.05, shot_seed=NOISE_SEED)


@pytest.mark.parametrize("kind", ["depol", "pauli", "shot"])
@pytest.mark.parametrize("n", [5, 10])
def test_noise_teacher_forced_and_the_counter(tq, n, kind):
    """K = 5: ids eval_base + 2k, + 2k + 1, + 2K; a second run on the handle starts from eval_base + 2K + 1; a refused
    call leaves the counter where it was; then an env-step, whose draws are numbered on the pre-action list."""
    K = 5
    rng = np.random.default_rng(900 + n)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 20, rng)
    circuits = []
    for b in range(3):
        g = random_gates(n, 14 + 4 * b, rng, p_cnot=0.3)
        circuits.append((with_noise_gates(*g[:4]), g[4]))
    eng = _engine(tq, n, ham, psi0)
    noise = _noise_setting(eng, kind)
    opts = dict(maxiter=K, seed=3)
    _run(tq, eng, circuits, opts, noise=noise, eval_base=0, psi0=psi0, ham=ham)
    with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:"):
        eng.batch_run_minimize_spsa(maxiter=K, a=0.0)
    with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:"):
        eng.batch_run_env_step_spsa(maxiter=K, beta_2=1.0)
    _run(tq, eng, circuits, opts, noise=noise, eval_base=2 * K + 1, psi0=psi0, ham=ham)
    new = [int(np.nonzero(circuits[0][0][0] == 0)[0][0]),                     # a CNOT (and its two-qubit channel)
           int(np.nonzero((circuits[1][0][0] >= 1) & (circuits[1][0][0] <= 3))[0][-1]),      # the last rotation
           -1]
    _run(tq, eng, circuits, opts, new_gates=new, env=True, noise=noise, eval_base=2 * (2 * K + 1), psi0=psi0, ham=ham)
    eng.close()


def test_shot_noise_alone(tq):
    """no Pauli noise: the noiseless instance with the Gaussian term keyed by the evaluation id"""
    n, K = 5, 5
    rng = np.random.default_rng(77)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 20, rng)
    g = random_gates(n, 16, rng, p_cnot=0.3)
    eng = _engine(tq, n, ham, psi0)
    eng.set_shot_noise(0.1, 99)
    noise = dict(seed=99, shot_sigma=0.1, shot_seed=99)
    _run(tq, eng, [(g[:4], g[4])] * 2, dict(maxiter=K, seed=1), noise=noise, eval_base=0, psi0=psi0, ham=ham)
    eng.close()


# ---- env-step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 12])
def test_env_step(tq, n):
    """lbfgs_helpers.envstep_case: the new gate is the last rotation (circuits 0..2), a CNOT (3: no hole), none (4); a
    circuit without rotations; and a rotation in the middle of the circuit.  K = 4, then K = 0."""
    case = lh.envstep_case(n)
    circuits = [(c["gates"], c["theta"]) for c in case["circuits"]]
    new = [c["new_gate"] for c in case["circuits"]]
    cn = (np.array([0, 0], np.int32), np.array([0, 1], np.int32), np.array([1, 0], np.int32), np.array([-1, -1], np.int32))
    circuits.append((cn, np.zeros(0)))                       # no rotation at all
    new.append(1)
    one = (np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.array([1, -1], np.int32), np.array([-1, 0], np.int32))
    circuits.append((one, np.array([0.0])))                  # its only rotation is the new gate: nothing to optimise
    new.append(1)
    g4, th4 = circuits[4]
    rot = np.nonzero(g4[0] != 0)[0]
    circuits.append((g4, th4))
    new.append(int(rot[rot.size // 2]))                      # the hole has variables on both sides
    eng = _engine(tq, n, case["ham"], case["psi0"])
    x, f, nfev = _run(tq, eng, circuits, dict(maxiter=4, seed=9), new_gates=new, env=True, psi0=case["psi0"], ham=case["ham"])
    assert list(nfev) == [8, 8, 8, 8, 8, 1, 1, 8]
    x0, f0, nfev0 = _run(tq, eng, circuits, dict(maxiter=0, seed=9), new_gates=new, env=True, psi0=case["psi0"], ham=case["ham"])
    assert list(nfev0) == [1] * 8
    assert np.array_equal(x0, np.concatenate([th for _, th in circuits]).astype(np.float32).astype(np.float64))
    eng.close()


def test_single_circuit_entry_point_and_k0(tq):
    case = lh.trajectory_case(4, 0, False)
    eng = _engine(tq, 4, case["ham"], case["psi0"])
    circ = tq.Circuit(*case["gates"], case["theta"].size)
    eng.set_circuit(circ)
    x, f, nfev = eng.minimize_spsa(case["theta"], maxiter=6, seed=2)
    eng.batch_load([circ], [case["theta"]])
    eng.batch_run_minimize_spsa(maxiter=6, seed=2)
    xb, fb, nb = eng.batch_fetch()
    assert np.array_equal(x, xb) and f == fb[0] and nfev == nb[0] == 13
    assert abs(f - lh.oracle_energy(case["psi0"], *case["gates"], x, case["ham"])) <= E_TOL
    x, f, nfev = eng.minimize_spsa(case["theta"], maxiter=0)
    assert np.array_equal(x, case["theta"]) and nfev == 1
    assert abs(f - lh.oracle_energy(case["psi0"], *case["gates"], case["theta"], case["ham"])) <= E_TOL
    assert eng.last_kernel_ms() > 0.0
    eng.close()


# ---- batch independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 12])
def test_batch_independence(tq, n):
    """Circuit b of a batch of 7 mixed circuits has the same bits as the same circuit at position b of a batch that
    fills the device (B from device_info), and other perturbations at another position."""
    rng = np.random.default_rng(31 + n)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 16, rng, real=False)
    circs, thetas = [], []
    for b in range(7):
        kind, q0, q1, pidx, th = random_gates(n, 5 + 6 * b, rng)
        circs.append(tq.Circuit(kind, q0, q1, pidx, th.size))
        thetas.append(th)
    eng = _engine(tq, n, ham, psi0)
    opts = dict(maxiter=3, seed=12)
    eng.batch_load(circs, thetas)
    eng.batch_run_minimize_spsa(**opts)
    x7, f7, n7 = eng.batch_fetch()
    info = eng.device_info()
    B = int(info["cu_count"]) * int(info["wg_per_cu"])
    assert 7 < B <= 4096
    pick = 5
    big_c = [circs[b] if b < 7 else circs[pick] for b in range(B)]
    big_t = [thetas[b] if b < 7 else thetas[pick] for b in range(B)]
    eng.batch_load(big_c, big_t)
    eng.batch_run_minimize_spsa(**opts)
    xB, fB, nB = eng.batch_fetch()
    assert np.array_equal(xB[:x7.size], x7) and np.array_equal(fB[:7], f7) and np.array_equal(nB[:7], n7)
    P = thetas[pick].size
    off = sum(t.size for t in thetas[:pick])
    tail = xB[x7.size:].reshape(B - 7, P)
    assert not np.array_equal(tail[0], x7[off:off + P]) and not np.array_equal(tail[0], tail[1])
    eng.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(tq):
    """Every refusal of the entry points; afterwards a COBYLA run equals the one of a fresh handle, bit for bit."""
    n = 6
    rng = np.random.default_rng(9)
    kind, q0, q1, pidx, th = random_gates(n, 20, rng)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 12, rng)
    circ = tq.Circuit(kind, q0, q1, pidx, th.size)

    def fresh():
        eng = _engine(tq, n, ham, psi0)
        eng.set_circuit(circ)
        return eng

    want = fresh().minimize_cobyla(th, 1.0, 1e-4, 60)

    def usable(eng):
        got = eng.minimize_cobyla(th, 1.0, 1e-4, 60)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]

    def refused(eng, code, words, call):
        with pytest.raises(tq.VQEError, match=rf"error {code}:") as err:
            call(eng)
        assert any(w in str(err.value) for w in words), str(err.value)

    single = lambda e: e.minimize_spsa(th, maxiter=3)
    for setup, undo, words in (
            (lambda e: e.set_noise_mode(1), lambda e: e.set_noise_mode(0), ("exact channel",)),
            (lambda e: e.set_term_shard(0, 2), lambda e: e.set_term_shard(0, 1), ("term-sharded",)),
            (lambda e: (e.set_noise_kraus(tq.channels.dephasing(0.2), None), e.set_kraus_traj(8)),
             lambda e: (e.set_kraus_traj(0), e.set_noise_kraus(None, None)), ("Kraus",))):
        eng = fresh()
        setup(eng)
        refused(eng, ESTATE, words, single)
        eng.batch_load([circ], [th])
        refused(eng, ESTATE, words, lambda e: e.batch_run_minimize_spsa(maxiter=3))
        refused(eng, ESTATE, words, lambda e: e.batch_run_env_step_spsa(maxiter=3))
        undo(eng)
        usable(eng)
    eng = fresh()
    for bad in (dict(maxiter=-1), dict(a=0.0), dict(c=-0.1), dict(eps=0.0), dict(alpha=-1.0), dict(gamma=-1.0),
                dict(lamda=-1.0), dict(stability=-1.0), dict(beta_1=1.0), dict(beta_2=-0.5), dict(a=float("nan")),
                dict(c=float("inf"))):
        refused(eng, EINVAL, ("Adam-SPSA",), lambda e, bad=bad: e.minimize_spsa(th, **bad))
    usable(eng)
    # n = 14 (streaming path): VQE_EINVAL; an amplitude shard can only be set there
    n14 = 14
    k14, a14, b14, p14, t14 = random_gates(n14, 10, rng)
    h14, psi14 = random_hamiltonian(n14, 6, rng), random_state(n14, rng)
    e14 = _engine(tq, n14, h14, psi14)
    e14_ref = vo.energy_pauli(vo.run_circuit(psi14, k14, a14, b14, p14, t14), *h14)
    e14.set_circuit(tq.Circuit(k14, a14, b14, p14, t14.size))
    refused(e14, EINVAL, ("n_qubits <= 13",), lambda e: e.minimize_spsa(t14, maxiter=2))
    e14.set_amplitude_shard(0, 2)
    refused(e14, ESTATE, ("amplitude shard",), lambda e: e.minimize_spsa(t14, maxiter=2))
    e14.set_amplitude_shard(0, 1)
    assert abs(e14.energy(t14) - e14_ref) <= E_TOL * lh.ham_scale(h14)
    e14.close()


# ---- environments ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    from helpers import make_data_root
    return make_data_root(str(tmp_path_factory.mktemp("dmrg-to-qc")))


SCRIPTS = [
    [0, 56 + 1 * 3 + 1, 56 + 1 * 3 + 0],      # CNOT(0->1), RY(q1), RX(q1)
    [56 + 2 * 3 + 1, 3, 56 + 5 * 3 + 0],
    [56 + 4 * 3 + 0, 56 + 6 * 3 + 1, 20],
]
ENV_SPSA = dict(maxiter=5, seed=21)


@pytest.mark.parametrize("cfg,module", [("TensorRL_fixed/H2O8q_TNbond2", "environment_qulacs_TN_notin_agent"),
                                        ("TensorRL_fixed/H2O8q_TNbond2_noise", "environment_qulacs_TN_notin_agent_noise")])
def test_vec_env_spsa_native_and_python_loops(data_root, cfg, module):
    """Three steps: both host loops identical, every energy the oracle's at the returned angles (the noisy class: one
    draw of the full circuit with id eval_base + 2K of that step's launch)."""
    import importlib

    import torch
    from helpers import load_case, oracle_init_state, reference_config
    from tensorrl_qas_amd.environments.utils.utils import dictionary_of_actions
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    cls = importlib.import_module("tensorrl_qas_amd.environments." + module).CircuitEnv
    conf = reference_config(cfg, data_root)
    conf["non_local_opt"]["global_iters"] = 40
    case = load_case("H2O_8q")
    dev = torch.device("cuda:0")
    B, K, seed = 3, ENV_SPSA["maxiter"], 4
    vn = VecCircuitEnv(cls, conf, dev, B, seed=seed, native=True, device_optimizer="spsa", spsa_opts=ENV_SPSA)
    vp = VecCircuitEnv(cls, conf, dev, B, seed=seed, native=False, device_optimizer="spsa", spsa_opts=ENV_SPSA)
    assert vn.native and not vp.native and vn.device_optimizer == "spsa"
    n = vn.num_qubits
    ham = (*vo.pauli_masks(case["paulis"], n, reverse=False), case["weights"])
    psi0 = oracle_init_state(case)
    table = dictionary_of_actions(n)
    assert torch.equal(vn.reset(), vp.reset())
    if cls.NOISY:      # reset() of the Python loop evaluates B energies, the native one none: align the trajectory counters
        for v in (vn, vp):
            v.engine.set_noise(cls.NOISE_P1, cls.NOISE_P2, seed)
    for t in range(3):
        acts = [table[s[t]] for s in SCRIPTS]
        on, rn, dn = vn.step(acts)
        op, rp, dp = vp.step(acts)
        assert torch.equal(on, op) and torch.equal(rn, rp) and dn == dp, t
        for b in range(B):
            w, e = vn.envs[b], vp.envs[b]
            assert (w.energy, w.nfev) == (e.energy, e.nfev) and w.rwd == float(e.rwd)
            assert torch.equal(w.state, e.state)
            assert e.nfev in (1, 2 * K)
            k, a, q, p, th = vo.ansatz_from_state(e.state.numpy(), n)
            if cls.NOISY:
                gates = with_noise_gates(k, a, q, p)
                codes, _ = npo.draws(seed, b, t * (2 * K + 1) + 2 * K, gates[0], None, None, cls.NOISE_P1, cls.NOISE_P2)
                ref = npo.energy(psi0, gates, th, ham, codes)
            else:
                ref = vo.energy_pauli(vo.run_circuit(psi0, k, a, q, p, th), *ham)
            assert abs(e.energy - ref) <= E_TOL, (t, b, e.energy, ref)
    vn.close()


def test_vec_env_spsa_refusals(data_root):
    import torch
    from helpers import reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv as NoisyEnv
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    import tensorrl_qas_amd as tq
    dev = torch.device("cuda:0")
    noisy = reference_config("TensorRL_fixed/H2O8q_TNbond2_noise", data_root)
    clean = reference_config("TensorRL_fixed/H2O8q_TNbond2", data_root)
    with pytest.raises((NotImplementedError, ValueError)):
        VecCircuitEnv(NoisyEnv, noisy, dev, 2, device_optimizer="spsa", noise_channel="exact")
    with pytest.raises((NotImplementedError, ValueError)):
        VecCircuitEnv(NoisyEnv, noisy, dev, 2, device_optimizer="spsa", noise_kraus=(tq.channels.dephasing(0.1), None),
                      kraus_trajectories=4)
    with pytest.raises((NotImplementedError, ValueError)):
        VecCircuitEnv(NoisyEnv, noisy, dev, 2, device_optimizer="spsa", noise_realisations=4)
    with pytest.raises(ValueError):
        VecCircuitEnv(CircuitEnv, clean, dev, 2, device_optimizer="adam")
    with pytest.raises(ValueError):
        VecCircuitEnv(CircuitEnv, clean, dev, 2, device_optimizer="cobyla", spsa_opts=dict(maxiter=3))
    with pytest.raises(TypeError):
        VecCircuitEnv(CircuitEnv, clean, dev, 2, device_optimizer="spsa", spsa_opts=dict(history=3))
    v = VecCircuitEnv(CircuitEnv, clean, dev, 2, device_optimizer="spsa")
    assert v._spsa_opts["maxiter"] == int(v._proto.global_iters) // 2      # nfev stays within COBYLA's budget
    v.close()


def test_circuit_env_adam_spsa_each_step(data_root):
    """method = adam_spsa_each_step: one batch_run_env_step_spsa per step on the config's own keys; the shipped zeros
    of a and c raise ValueError naming the key."""
    import torch
    from helpers import load_case, oracle_init_state, reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    from tensorrl_qas_amd.environments.utils.utils import dictionary_of_actions
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2", data_root)
    conf["non_local_opt"]["method"] = "adam_spsa_each_step"
    dev = torch.device("cuda:0")
    assert float(conf["non_local_opt"]["a"]) == 0.0 and float(conf["non_local_opt"]["c"]) == 0.0
    with pytest.raises(ValueError, match=r"non_local_opt\.a"):
        CircuitEnv(conf, dev)
    conf["non_local_opt"]["a"] = 0.1
    with pytest.raises(ValueError, match=r"non_local_opt\.c"):
        CircuitEnv(conf, dev)
    conf["non_local_opt"]["c"] = 0.1
    conf["non_local_opt"]["global_iters"] = 12
    conf["non_local_opt"]["maxfev"] = 0
    env = CircuitEnv(conf, dev)
    assert env._spsa_opts["maxiter"] == 6 and env.optimizer_kind == "device_spsa"
    conf["non_local_opt"]["maxfev"] = 8
    env = CircuitEnv(conf, dev)
    assert env._spsa_opts["maxiter"] == 4
    env.reset()
    case = load_case("H2O_8q")
    n = env.num_qubits
    ham = (*vo.pauli_masks(case["paulis"], n, reverse=False), case["weights"])
    psi0 = oracle_init_state(case)
    table = dictionary_of_actions(n)
    for ai in SCRIPTS[0]:
        obs, rwd, done = env.step(table[ai])
        k, a, q, p, th = vo.ansatz_from_state(env.state.numpy(), n)
        assert abs(env.energy - vo.energy_pauli(vo.run_circuit(psi0, k, a, q, p, th), *ham)) <= E_TOL
        assert env.nfev in (1, 8) and torch.isfinite(rwd)
