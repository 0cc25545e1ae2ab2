"""GPU: the device L-BFGS (k_lds_minimize_lbfgs; vqe_minimize_lbfgs, vqe_batch_run_minimize_lbfgs, vqe_batch_run_env_step_lbfgs)
against its numpy restatement on the CPU oracle (tests/lbfgs_helpers.py), trial point by trial point, and the
VecCircuitEnv that steps with it.  tests/test_lbfgs_cpu.py checks on the CPU that no compared case has a marginal
decision."""
import numpy as np
import pytest

import lbfgs_helpers as lh
import vqe_oracle as vo
from helpers import fermionic_hamiltonian, random_gates, random_hamiltonian, random_state

pytestmark = pytest.mark.gpu

X_TOL = lh.X_TOL      # trial points: 1e-9
F_TOL = 1e-10         # energies, times scale = max(1, sum |c_k|)


def _engine(n, ham, psi0):
    import tensorrl_qas_amd as tq
    eng = tq.VQEEngine(n, 0)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    return eng


def _circ(gates, P):
    import tensorrl_qas_amd as tq
    return tq.Circuit(*gates, P)


def _traced_run(eng, gates, theta, **opts):
    """One circuit through the batch entry points with the trace on -> (x, f, nfev, nit, status, trace f, trace x)"""
    eng.batch_load([_circ(gates, theta.size)], [theta])
    eng.batch_set_trace(True)
    eng.batch_run_minimize_lbfgs(**opts)
    x, f, nfev = eng.batch_fetch()
    nit, st = eng.batch_fetch_lbfgs_info()
    tf, tx = eng.batch_fetch_trace(0, theta.size)
    eng.batch_set_trace(False)
    return x, float(f[0]), int(nfev[0]), int(nit[0]), int(st[0]), tf, tx


def _assert_matches(case, ref, got):
    x, f, nfev, nit, st, tf, tx = got
    assert ref.marginal == []
    assert (nfev, nit, st) == (ref.nfev, ref.nit, ref.status)
    assert np.all(tf[nfev:] == 0.0) and np.all(tx[nfev:] == 0.0)
    for k, t in enumerate(ref.trials):
        assert np.abs(tx[k] - t.x).max(initial=0.0) <= X_TOL, (k, np.abs(tx[k] - t.x).max())
        e = lh.oracle_energy(case["psi0"], *case["gates"], tx[k], case["ham"])
        assert abs(tf[k] - e) <= F_TOL * case["scale"], (k, tf[k], e)
    assert np.abs(x - ref.x).max(initial=0.0) <= X_TOL
    assert abs(f - ref.f) <= 2 * F_TOL * case["scale"]


@pytest.mark.parametrize("key", lh.trajectory_cases(), ids=lambda k: f"n{k[0]}-h{k[1]}-{'su4' if k[2] else 'rot'}")
def test_trajectory_parity(key):
    """history = 3, maxiter = 6 (the oldest pair leaves inside the run): every evaluation's point and value, the
    counts and the status equal the restatement's.  n = 13 runs the LAM_GLOBAL instantiation."""
    case = lh.trajectory_case(*key)
    ref = lh.restated(("traj", key), case, **lh.TRAJ_OPTS)
    eng = _engine(case["n"], case["ham"], case["psi0"])
    _assert_matches(case, ref, _traced_run(eng, case["gates"], case["theta"], **lh.TRAJ_OPTS))


def test_persistent_grid_reuses_its_scratch_slice():
    """n = 13 (lambda in global scratch, persistent grid of CUs x workgroups per CU): with grid + 3 circuits the first
    three workgroups run a second circuit in the slice their first one used - the twin of that first one, and the
    results must be the same bit for bit."""
    case = lh.trajectory_case(13, 0, False)
    eng = _engine(13, case["ham"], case["psi0"])
    circ = _circ(case["gates"], case["theta"].size)
    eng.batch_load([circ], [case["theta"]])
    eng.batch_run_minimize_lbfgs(history=3, maxiter=2)
    info = eng.device_info()
    grid = int(info["cu_count"]) * int(info["wg_per_cu"])
    assert 1 <= grid <= 4096
    rng = np.random.default_rng(3)
    thetas = [case["theta"] + 0.3 * rng.normal(size=case["theta"].size) for _ in range(grid)]
    thetas += [t.copy() for t in thetas[:3]]
    B = grid + 3
    eng.batch_load([circ] * B, thetas)
    eng.batch_run_minimize_lbfgs(history=3, maxiter=2)
    x, f, nfev = eng.batch_fetch()
    nit, st = eng.batch_fetch_lbfgs_info()
    x = x.reshape(B, -1)
    for i in range(3):
        assert np.array_equal(x[grid + i], x[i]) and f[grid + i] == f[i]
        assert (nfev[grid + i], nit[grid + i], st[grid + i]) == (nfev[i], nit[i], st[i])
    assert not np.array_equal(x[0], x[1])
    assert np.all(nit >= 1) and np.all(f <= eng_energy_upper(case))
    # one of them against the oracle
    e = lh.oracle_energy(case["psi0"], *case["gates"], x[grid + 1], case["ham"])
    assert abs(f[grid + 1] - e) <= F_TOL * case["scale"]


def eng_energy_upper(case):
    return float(np.abs(case["ham"][2]).sum())


def _line_searches(tx, nfev):
    """Split the traced points into line searches: inside one, every trial halves the step of the one before
    (x_j - base = (x_{j-1} - base) / 2).  -> list of (first, last) evaluation indices; base of a search = the last
    point of the search before it (the accepted one)."""
    out, base, i = [], tx[0], 1
    while i < nfev:
        j = i
        while j + 1 < nfev and np.allclose(tx[j + 1] - base, 0.5 * (tx[j] - base), rtol=1e-9, atol=1e-14):
            j += 1
        out.append((i, j))
        base = tx[j]
        i = j + 1
    return out


def test_monotone_and_terminal_properties():
    """n = 8, about 30 parameters, default options."""
    n = 8
    rng = np.random.default_rng(21)
    gates = random_gates(n, 45, rng, p_cnot=0.3)
    theta = gates[4]
    gates = gates[:4]
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 22, rng, real=False)
    assert 24 <= theta.size <= 38
    eng = _engine(n, ham, psi0)
    x, f, nfev, nit, st, tf, tx = _traced_run(eng, gates, theta)
    assert st in (lh.GTOL, lh.FTOL, lh.LINESEARCH, lh.MAXFUN, lh.MAXITER)
    assert 1 <= nit <= 100 and nit < nfev <= 1000
    searches = _line_searches(tx, nfev)
    accepted = [0] + [j for _, j in searches]
    if st in (lh.LINESEARCH, lh.MAXFUN) and len(accepted) > nit + 1:
        accepted = accepted[:-1]                      # the last search ended without an accepted trial
    assert len(accepted) == nit + 1
    fa = tf[accepted]
    assert np.all(fa[1:] <= fa[:-1]), "the accepted energies must never increase"
    assert f == fa[-1] and np.array_equal(x, tx[accepted[-1]])
    eng.set_circuit(_circ(gates, theta.size))
    e, g = eng.energy_grad(x)
    if st == lh.GTOL:
        assert np.abs(g).max() <= lh.DEFAULTS["gtol"]
    assert abs(f - eng.energy(x)) <= 1e-12
    assert f < tf[0] - 1e-3                           # it did minimise


def test_shared_and_unused_parameters():
    case = lh.shared_unused_case()
    ref = lh.restated("shared", case, **lh.TRAJ_OPTS)
    eng = _engine(case["n"], case["ham"], case["psi0"])
    got = _traced_run(eng, case["gates"], case["theta"], **lh.TRAJ_OPTS)
    _assert_matches(case, ref, got)
    assert np.all(got[6][:got[2], 2] == case["theta"][2])      # the unused parameter never moves, in any trial point
    assert got[0][2] == case["theta"][2]


@pytest.mark.parametrize("n", [6, 12])
def test_batch_of_unequal_circuits_equals_single_runs(n):
    import tensorrl_qas_amd as tq
    rng = np.random.default_rng(31 + n)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, n_hop=2 * n, n_quad=n, rng=rng, dressed=1)
    circs, thetas = [], []
    for b in range(7):
        kind, q0, q1, pidx, th = random_gates(n, 5 + 9 * b, rng)
        circs.append(tq.Circuit(kind, q0, q1, pidx, th.size))
        thetas.append(th)
    eng = _engine(n, ham, psi0)
    opts = dict(maxiter=5, history=4)
    eng.batch_load(circs, thetas)
    eng.batch_run_minimize_lbfgs(**opts)
    x, f, nfev = eng.batch_fetch()
    nit, st = eng.batch_fetch_lbfgs_info()
    xraw = eng.batch_fetch_xopt()
    assert np.array_equal(x, xraw)                    # no float32 rounding outside an environment step
    off = 0
    for b, (c, th) in enumerate(zip(circs, thetas)):
        eng.set_circuit(c)
        x1, f1, nfev1, nit1, st1 = eng.minimize_lbfgs(th, **opts)
        assert np.array_equal(x[off:off + th.size], x1) and f[b] == f1
        assert (nfev[b], nit[b], st[b]) == (nfev1, nit1, st1)
        off += th.size
    assert off == x.size


@pytest.mark.parametrize("n", [6, 12])
def test_env_step(n):
    """The rule of the COBYLA env-step: the optimiser sees the pre-action circuit, xopt is its optimum (the new gate's
    angle untouched), x = float32(xopt), f the energy of the FULL circuit at x."""
    import tensorrl_qas_amd as tq
    case = lh.envstep_case(n)
    cs = case["circuits"]
    eng = _engine(n, case["ham"], case["psi0"])
    eng.batch_load([tq.Circuit(*c["gates"], c["theta"].size) for c in cs], [c["theta"] for c in cs])
    eng.batch_set_new_gate([c["new_gate"] for c in cs])
    eng.batch_run_env_step_lbfgs(**lh.TRAJ_OPTS)
    x, f, nfev = eng.batch_fetch()
    xopt = eng.batch_fetch_xopt()
    nit, st = eng.batch_fetch_lbfgs_info()
    off = 0
    for b, c in enumerate(cs):
        P = c["theta"].size
        xb, xo = x[off:off + P], xopt[off:off + P]
        off += P
        ref, hole = lh.envstep_restated(n, b)
        assert ref.marginal == []
        keep = np.arange(P) != hole
        assert np.abs(xo[keep] - ref.x).max(initial=0.0) <= X_TOL, (b, np.abs(xo[keep] - ref.x).max())
        assert (nfev[b], nit[b], st[b]) == (ref.nfev, ref.nit, ref.status)
        if hole >= 0:
            assert xo[hole] == c["theta"][hole]
        assert np.array_equal(xb, xo.astype(np.float32).astype(np.float64))
        e = lh.oracle_energy(case["psi0"], *c["gates"], xb, case["ham"])
        assert abs(f[b] - e) <= F_TOL * case["scale"], (b, f[b], e)


def test_env_step_trace_with_the_new_gate_in_the_middle():
    """The new gate's parameter has variables on both sides: the trace holds the points of the pre-action circuit (the
    hole closed up, P - 1 entries), xopt keeps the hole at its theta0 value."""
    import tensorrl_qas_amd as tq
    full, sub, hole = lh.envstep_middle_case()
    ref = lh.restated("envstep-middle", sub, **lh.TRAJ_OPTS)
    assert ref.marginal == []
    P = full["theta"].size
    eng = _engine(6, full["ham"], full["psi0"])
    eng.batch_load([tq.Circuit(*full["gates"], P)], [full["theta"]])
    eng.batch_set_new_gate([full["new_gate"]])
    eng.batch_set_trace(True)
    eng.batch_run_env_step_lbfgs(**lh.TRAJ_OPTS)
    x, f, nfev = eng.batch_fetch()
    xopt = eng.batch_fetch_xopt()
    nit, st = eng.batch_fetch_lbfgs_info()
    tf, tx = eng.batch_fetch_trace(0, P)
    eng.batch_set_trace(False)
    assert (nfev[0], nit[0], st[0]) == (ref.nfev, ref.nit, ref.status)
    assert np.all(tf[ref.nfev:] == 0.0) and np.all(tx[ref.nfev:] == 0.0)
    for k, t in enumerate(ref.trials):
        assert np.abs(tx[k, :P - 1] - t.x).max() <= X_TOL, (k, np.abs(tx[k, :P - 1] - t.x).max())
        assert tx[k, P - 1] == 0.0
        e = lh.oracle_energy(sub["psi0"], *sub["gates"], tx[k, :P - 1], sub["ham"])
        assert abs(tf[k] - e) <= F_TOL * sub["scale"], (k, tf[k], e)
    keep = np.arange(P) != hole
    assert np.abs(xopt[keep] - ref.x).max() <= X_TOL and xopt[hole] == full["theta"][hole]
    assert np.array_equal(x, xopt.astype(np.float32).astype(np.float64))
    e = lh.oracle_energy(full["psi0"], *full["gates"], x, full["ham"])
    assert abs(f[0] - e) <= F_TOL * full["scale"]


def test_lbfgs_info_goes_stale_with_the_next_cobyla_run():
    import tensorrl_qas_amd as tq
    case = lh.shared_unused_case()
    eng = _engine(case["n"], case["ham"], case["psi0"])
    eng.batch_load([_circ(case["gates"], case["theta"].size)], [case["theta"]])
    eng.batch_run_minimize_lbfgs(maxiter=1)
    assert eng.batch_fetch_lbfgs_info()[0][0] == 1
    eng.batch_run_minimize(maxfun=20)
    with pytest.raises(tq.VQEError, match=r"error -1:"):
        eng.batch_fetch_lbfgs_info()
    eng.batch_run_minimize_lbfgs(maxiter=2)
    assert eng.batch_fetch_lbfgs_info()[0][0] == 2


def test_refusals_leave_the_handle_usable():
    import tensorrl_qas_amd as tq
    n = 6
    rng = np.random.default_rng(9)
    kind, q0, q1, pidx, th = random_gates(n, 20, rng)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 12, rng)
    circ = tq.Circuit(kind, q0, q1, pidx, th.size)
    e_ref = vo.energy_pauli(vo.run_circuit(psi0, kind, q0, q1, pidx, th), *ham)
    ESTATE, EINVAL = -1, -22

    def fresh():
        eng = _engine(n, ham, psi0)
        eng.set_circuit(circ)
        return eng

    def refused(eng, code, call, undo=lambda e: None):
        with pytest.raises(tq.VQEError, match=rf"error {code}:"):
            call(eng)
        undo(eng)
        assert abs(eng.energy(th) - e_ref) <= 1e-10
        x, f, nfev, nit, st = eng.minimize_lbfgs(th, maxiter=2)
        assert f < e_ref and nit >= 1

    single = lambda e: e.minimize_lbfgs(th)
    for setup, undo in ((lambda e: e.set_noise(0.01, 0.0, 1), lambda e: e.set_noise(0.0, 0.0, 1)),
                        (lambda e: e.set_noise_mode(1), lambda e: e.set_noise_mode(0)),
                        (lambda e: e.set_shot_noise(0.1, 3), lambda e: e.set_shot_noise(0.0, 3)),
                        (lambda e: e.set_term_shard(0, 2), lambda e: e.set_term_shard(0, 1))):
        eng = fresh()
        setup(eng)
        refused(eng, ESTATE, single, undo)
    # the batch entry points refuse in the same way
    eng = fresh()
    eng.batch_load([circ], [th])
    eng.set_shot_noise(0.1, 3)
    for call in (lambda e: e.batch_run_minimize_lbfgs(), lambda e: e.batch_run_env_step_lbfgs()):
        with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
            call(eng)
    eng.set_shot_noise(0.0, 3)
    eng.batch_run_energy()
    assert abs(eng.batch_fetch(want_x=False)[1][0] - e_ref) <= 1e-10
    assert abs(eng.energy(th) - e_ref) <= 1e-10
    eng.batch_load([circ], [th])
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
        eng.batch_fetch_lbfgs_info()                  # no L-BFGS run on this batch yet
    eng.batch_run_minimize_lbfgs(maxiter=1)
    assert eng.batch_fetch_lbfgs_info()[0][0] == 1
    # bad options
    eng = fresh()
    for bad in (dict(history=0), dict(history=17), dict(maxiter=-1), dict(maxfun=0), dict(gtol=-1e-3), dict(ftol=-1.0),
                dict(c1=0.0), dict(c1=1.0)):
        refused(eng, EINVAL, lambda e, bad=bad: e.minimize_lbfgs(th, **bad))
    # n = 14 (streaming path): no adjoint kernel; an amplitude shard can only be set there
    n14 = 14
    k14, a14, b14, p14, t14 = random_gates(n14, 10, rng)
    h14 = random_hamiltonian(n14, 6, rng)
    psi14 = random_state(n14, rng)
    e14 = _engine(n14, h14, psi14)
    e14_ref = vo.energy_pauli(vo.run_circuit(psi14, k14, a14, b14, p14, t14), *h14)
    e14.set_circuit(tq.Circuit(k14, a14, b14, p14, t14.size))
    with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:"):
        e14.minimize_lbfgs(t14)
    assert abs(e14.energy(t14) - e14_ref) <= 1e-10 * lh.ham_scale(h14)
    e14.set_amplitude_shard(0, 2)
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
        e14.minimize_lbfgs(t14)
    e14.set_amplitude_shard(0, 1)
    assert abs(e14.energy(t14) - e14_ref) <= 1e-10 * lh.ham_scale(h14)


# ---- VecCircuitEnv(device_optimizer="lbfgs") -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    from helpers import make_data_root
    return make_data_root(str(tmp_path_factory.mktemp("dmrg-to-qc")))


SCRIPTS = [
    [0, 56 + 1 * 3 + 1, 56 + 1 * 3 + 0, 7 + 1, 56 + 3 * 3 + 2, 56 + 0 * 3 + 1],      # CNOT(0->1), RY(q1), RX(q1), CNOT(1->3), RZ(q3), RY(q0)
    [56 + 2 * 3 + 1, 3, 56 + 5 * 3 + 0, 56 + 2 * 3 + 2, 8 + 4, 56 + 7 * 3 + 1],
    [56 + 4 * 3 + 0, 56 + 6 * 3 + 1, 20, 56 + 4 * 3 + 2, 56 + 0 * 3 + 0, 30],
]
ENV_OPTS = dict(history=3, maxiter=6)


def _restated_step(prev_state, state, n, psi0, ham, maxfun):
    """CircuitEnv.step restated on the oracle as _oracle_step of test_grad_gpu.py does, with the restated L-BFGS in
    scipy's place: it minimises the pre-action circuit, the optimum is rounded to float32 and the full circuit is
    evaluated at those angles.  -> (energy, nfev)"""
    import torch
    k, a, b, p, th = vo.ansatz_from_state(prev_state.numpy(), n)
    if th.size == 0:
        xo, nfev = th, 1
    else:
        r = lh.lbfgs(lh.oracle_fun(psi0, k, a, b, p, th.size, ham), th, scale=lh.ham_scale(ham), maxfun=maxfun, **ENV_OPTS)
        xo, nfev = r.x, r.nfev
    s = state.clone()
    rot = prev_state[:, n:n + 3] == 1
    ang = s[:, n + 3:]
    ang[rot] = torch.tensor(xo, dtype=torch.float)
    k2, a2, b2, p2, th2 = vo.ansatz_from_state(s.numpy(), n)
    return vo.energy_pauli(vo.run_circuit(psi0, k2, a2, b2, p2, th2), *ham), nfev


def test_vec_env_lbfgs_native_and_python_loops(data_root):
    import torch
    from helpers import load_case, oracle_init_state, reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    from tensorrl_qas_amd.environments.utils.utils import dictionary_of_actions
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2", data_root)
    conf["non_local_opt"]["global_iters"] = 40
    case = load_case("H2O_8q")
    dev = torch.device("cuda:0")
    B = 3
    vn = VecCircuitEnv(CircuitEnv, conf, dev, B, native=True, device_optimizer="lbfgs", lbfgs_opts=ENV_OPTS)
    vp = VecCircuitEnv(CircuitEnv, conf, dev, B, native=False, device_optimizer="lbfgs", lbfgs_opts=ENV_OPTS)
    assert vn.native and not vp.native
    n = vn.num_qubits
    ham = (*vo.pauli_masks(case["paulis"], n, reverse=False), case["weights"])
    psi0 = oracle_init_state(case)
    table = dictionary_of_actions(n)
    assert torch.equal(vn.reset(), vp.reset())
    for t in range(6):
        acts = [table[s[t]] for s in SCRIPTS]
        prev = [vp.envs[b].state.clone() for b in range(B)]
        on, rn, dn = vn.step(acts)
        op, rp, dp = vp.step(acts)
        assert torch.equal(on, op) and torch.equal(rn, rp) and dn == dp, t
        for b in range(B):
            w, e = vn.envs[b], vp.envs[b]
            assert (w.energy, w.nfev) == (e.energy, e.nfev) and w.rwd == float(e.rwd)
            assert torch.equal(w.state, e.state)
            e_ref, nfev_ref = _restated_step(prev[b], e.state, n, psi0, ham, 40)
            assert abs(e.energy - e_ref) <= 1e-8, (t, b, e.energy, e_ref)
            assert e.nfev == nfev_ref, (t, b, e.nfev, nfev_ref)
            assert 1 <= e.nfev <= 40


def test_vec_env_lbfgs_refuses_noisy_configs(data_root):
    import torch
    from helpers import reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2_noise", data_root)
    with pytest.raises(NotImplementedError):
        VecCircuitEnv(CircuitEnv, conf, torch.device("cuda:0"), 2, device_optimizer="lbfgs")
    with pytest.raises(ValueError):
        VecCircuitEnv(CircuitEnv, conf, torch.device("cuda:0"), 2, device_optimizer="adam")


@pytest.mark.parametrize("native", [True, False])
def test_vec_env_default_optimizer_is_unchanged(data_root, native):
    import torch
    from helpers import reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    from tensorrl_qas_amd.environments.utils.utils import dictionary_of_actions
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2", data_root)
    conf["non_local_opt"]["global_iters"] = 40
    dev = torch.device("cuda:0")
    plain = VecCircuitEnv(CircuitEnv, conf, dev, 3, native=native)
    named = VecCircuitEnv(CircuitEnv, conf, dev, 3, native=native, device_optimizer="cobyla")
    table = dictionary_of_actions(plain.num_qubits)
    assert torch.equal(plain.reset(), named.reset())
    for t in range(6):
        acts = [table[s[t]] for s in SCRIPTS]
        o1, r1, d1 = plain.step(acts)
        o2, r2, d2 = named.step(acts)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and d1 == d2
        for b in range(3):
            assert plain.envs[b].energy == named.envs[b].energy and plain.envs[b].nfev == named.envs[b].nfev
