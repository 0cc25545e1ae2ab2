"""GPU: the device L-BFGS on the streaming path (n >= 14; k_sl_step of csrc/vqe_stream_lbfgs.h between two
stream_energy_grad evaluations, behind vqe_set_stream_lbfgs) against the numpy restatement of tests/lbfgs_helpers.py on
the CPU oracle, against the library's own single runs, and under a VecCircuitEnv at 14 qubits.
tests/test_stream_lbfgs_cpu.py checks on the CPU that no compared case has a marginal decision.  Tolerances are those
of tests/test_lbfgs_gpu.py: 1e-9 on points, 1e-10 max(1, sum |c_k|) on energies."""
import numpy as np
import pytest

import lbfgs_helpers as lh
import stream_lbfgs_helpers as sh
import vqe_oracle as vo
from helpers import random_gates, random_hamiltonian, random_state

pytestmark = pytest.mark.gpu

X_TOL = lh.X_TOL
F_TOL = 1e-10
ESTATE, EINVAL = -1, -22


def _engine(n, ham, psi0, stream_lbfgs=True):
    import tensorrl_qas_amd as tq
    eng = tq.VQEEngine(n, 0)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    if stream_lbfgs:
        eng.set_stream_lbfgs()
    return eng


def _circ(gates, P):
    import tensorrl_qas_amd as tq
    return tq.Circuit(*gates, P)


# a circuit without a rotation (P = 0): one evaluation, status 0
_NO_ROT = (np.array([0, 0], np.int32), np.array([0, 5], np.int32), np.array([1, 2], np.int32), np.array([-1, -1], np.int32))


def _batch():
    """batch_case() plus the circuit without a rotation -> (case, circuits, thetas)"""
    import tensorrl_qas_amd as tq
    case = sh.batch_case()
    circs = [tq.Circuit(*c["gates"], c["theta"].size) for c in case["circuits"]] + [tq.Circuit(*_NO_ROT, 0)]
    thetas = [c["theta"] for c in case["circuits"]] + [np.zeros(0)]
    return case, circs, thetas


@pytest.mark.parametrize("n,seed", sh.CASES)
def test_prefix_parity(n, seed):
    """maxfun = k for k = 1 .. nfev: the counts and the status equal the restatement's, the point is its point, the
    value the oracle's energy there.  k = 1 is x0 itself with status 3."""
    case = sh.single_case(n, seed)
    full = sh.restated_single(n, seed)
    assert full.marginal == []
    eng = _engine(n, case["ham"], case["psi0"])
    eng.set_circuit(_circ(case["gates"], case["theta"].size))
    for k in range(1, full.nfev + 1):
        ref = sh.restated_single(n, seed, maxfun=k)
        x, f, nfev, nit, st = eng.minimize_lbfgs(case["theta"], **{**sh.TRAJ_OPTS, "maxfun": k})
        dx = np.abs(x - ref.x).max(initial=0.0)
        e = lh.oracle_energy(case["psi0"], *case["gates"], x, case["ham"])
        print(f"n={n} seed={seed} k={k}: (nfev, nit, status)=({nfev}, {nit}, {st}) |dx|={dx:.2e} |f-E(x)|={abs(f - e):.2e}")
        assert (nfev, nit, st) == (ref.nfev, ref.nit, ref.status), k
        assert dx <= X_TOL, (k, dx)
        assert abs(f - e) <= F_TOL * case["scale"], (k, f, e)
        if k == 1:
            assert np.array_equal(x, case["theta"]) and st == lh.MAXFUN


def test_batch_of_unequal_circuits_equals_single_runs():
    """Streams that stop at different evaluations (one of them past the host's look at the running count), and one
    without a parameter: every stream is what its circuit gives alone, bit for bit."""
    case, circs, thetas = _batch()
    eng = _engine(case["n"], case["ham"], case["psi0"])
    eng.batch_load(circs, thetas)
    eng.batch_run_minimize_lbfgs(**sh.BATCH_OPTS)
    x, f, nfev = eng.batch_fetch()
    nit, st = eng.batch_fetch_lbfgs_info()
    assert np.array_equal(x, eng.batch_fetch_xopt())           # no float32 rounding outside an environment step
    assert (nfev[4], nit[4], st[4]) == (1, 0, lh.GTOL)
    assert len(set(nfev[:4].tolist())) > 1 and nfev.max() > sh.STREAM_POLL, nfev
    off = 0
    for b, (c, th) in enumerate(zip(circs, thetas)):
        eng.set_circuit(c)
        x1, f1, nfev1, nit1, st1 = eng.minimize_lbfgs(th, **sh.BATCH_OPTS)
        assert np.array_equal(x[off:off + th.size], x1) and f[b] == f1, b
        assert (nfev[b], nit[b], st[b]) == (nfev1, nit1, st1), b
        off += th.size
    assert off == x.size
    e = vo.energy_pauli(vo.run_circuit(case["psi0"], *_NO_ROT, np.zeros(0)), *case["ham"])
    assert abs(f[4] - e) <= F_TOL * case["scale"]


def test_env_step():
    """The rule of the streaming COBYLA env-step: the optimiser sees the pre-action circuit, xopt is its optimum (the
    new gate's angle untouched), x = float32(xopt), f the energy of the FULL circuit at x; the states left behind are
    those of that last energy, so a reduction-only launch is accepted."""
    import tensorrl_qas_amd as tq
    case, circs, thetas = _batch()
    new_gate = sh.batch_new_gates() + [-1]
    eng = _engine(case["n"], case["ham"], case["psi0"])
    eng.batch_load(circs, thetas)
    eng.batch_set_new_gate(new_gate)
    eng.batch_run_env_step_lbfgs(**sh.BATCH_OPTS)
    x, f, nfev = eng.batch_fetch()
    xopt = eng.batch_fetch_xopt()
    nit, st = eng.batch_fetch_lbfgs_info()
    eng.batch_run_reduction()                                   # accepted: the last launch was an energy
    assert np.abs(eng.batch_fetch(want_x=False)[1] - f).max() <= F_TOL * case["scale"]
    gates = [c["gates"] for c in case["circuits"]] + [_NO_ROT]
    off = 0
    for b, th in enumerate(thetas):
        P = th.size
        xb, xo = x[off:off + P], xopt[off:off + P]
        off += P
        pre, x0, hole = lh.pre_action(*gates[b], th, new_gate[b])
        assert (hole >= 0) == (b in (0, 3))
        eng.set_circuit(tq.Circuit(*pre, x0.size))
        x1, f1, nfev1, nit1, st1 = eng.minimize_lbfgs(x0, **sh.BATCH_OPTS)
        keep = np.arange(P) != hole
        assert np.array_equal(xo[keep], x1), b
        assert (nfev[b], nit[b], st[b]) == (nfev1, nit1, st1), b
        if hole >= 0:
            assert xo[hole] == th[hole]
        assert np.array_equal(xb, xo.astype(np.float32).astype(np.float64))
        e = lh.oracle_energy(case["psi0"], *gates[b], xb, case["ham"])
        assert abs(f[b] - e) <= F_TOL * case["scale"], (b, f[b], e)
    # after a plain minimise run the last launch was a gradient: the states are the undone ones
    eng.batch_load(circs, thetas)
    eng.batch_run_minimize_lbfgs(maxiter=1)
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
        eng.batch_run_reduction()


def test_terminal_properties():
    """n = 14, seed 614 (18 parameters), default options."""
    n, seed = sh.CASES[0]
    case = sh.single_case(n, seed)
    th, scale = case["theta"], case["scale"]
    energy = lambda x: lh.oracle_energy(case["psi0"], *case["gates"], x, case["ham"])
    eng = _engine(n, case["ham"], case["psi0"])
    eng.set_circuit(_circ(case["gates"], th.size))
    x, f, nfev, nit, st = eng.minimize_lbfgs(th)
    print(f"default options: nfev={nfev} nit={nit} status={st} f={f:.12f} E(x0)={energy(th):.12f}")
    assert st in (lh.GTOL, lh.FTOL, lh.LINESEARCH, lh.MAXFUN, lh.MAXITER)
    assert 1 <= nit <= 100 and nit < nfev <= 1000
    assert f < energy(th) - 1e-3
    assert abs(f - energy(x)) <= F_TOL * scale
    eng.set_stream_grad()
    e, g = eng.energy_grad(x)
    assert abs(e - f) <= F_TOL * scale
    if st == lh.GTOL:
        assert np.abs(g).max() <= lh.DEFAULTS["gtol"]
    for k in (5, 9):                                            # one below and one above the host's polling interval
        xk, fk, nfk, nitk, stk = eng.minimize_lbfgs(th, maxfun=k)
        assert nfk <= k and (stk != lh.MAXFUN or nfk == k), (k, nfk, stk)
        if nfev > k:                                            # the unlimited run went on: this one ran out of evaluations
            assert (nfk, stk) == (k, lh.MAXFUN), (k, nfk, stk)
        assert abs(fk - energy(xk)) <= F_TOL * scale
    x0, f0, nf0, nit0, st0 = eng.minimize_lbfgs(th, maxiter=0)
    assert np.array_equal(x0, th) and (nf0, nit0, st0) == (1, 0, lh.MAXITER)
    assert abs(f0 - energy(th)) <= F_TOL * scale


def test_run_state_does_not_leak():
    import tensorrl_qas_amd as tq
    case, circs, thetas = _batch()
    eng = _engine(case["n"], case["ham"], case["psi0"])

    def lbfgs_run():
        eng.batch_load(circs, thetas)
        eng.batch_run_minimize_lbfgs(**sh.BATCH_OPTS)
        return (*eng.batch_fetch(), *eng.batch_fetch_lbfgs_info())

    first, second = lbfgs_run(), lbfgs_run()
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    # a shorter run after a longer one: nothing of the earlier records shows
    eng.batch_load(circs, thetas)
    eng.batch_run_minimize_lbfgs(history=2, maxiter=1)
    nit, st = eng.batch_fetch_lbfgs_info()
    assert list(nit[:4]) == [1, 1, 1, 1] and nit[4] == 0
    assert all(np.array_equal(a, b) for a, b in zip(first, lbfgs_run()))

    def cobyla_run(e):
        e.batch_load(circs, thetas)
        e.batch_run_minimize(maxfun=12)
        return e.batch_fetch()

    after = cobyla_run(eng)
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
        eng.batch_fetch_lbfgs_info()
    fresh = cobyla_run(_engine(case["n"], case["ham"], case["psi0"], stream_lbfgs=False))
    assert all(np.array_equal(a, b) for a, b in zip(after, fresh))


def test_one_driver_serves_both_optimisers_on_one_handle():
    """L-BFGS, COBYLA, L-BFGS on one handle: the two optimisers share the host's lock-step loop, its result buffers and
    its count of running streams, and nothing of a run shows in the next one."""
    case, circs, thetas = _batch()
    eng = _engine(case["n"], case["ham"], case["psi0"])

    def lbfgs_run():
        eng.batch_load(circs, thetas)
        eng.batch_run_minimize_lbfgs(**sh.BATCH_OPTS)
        return (*eng.batch_fetch(), *eng.batch_fetch_lbfgs_info())

    def cobyla_run(e):
        e.batch_load(circs, thetas)
        e.batch_run_minimize(maxfun=12)
        return (*e.batch_fetch(), e.batch_fetch_xopt())

    first, between, again = lbfgs_run(), cobyla_run(eng), lbfgs_run()
    assert all(np.array_equal(a, b) for a, b in zip(first, again))          # x, f, nfev, nit, status
    fresh = cobyla_run(_engine(case["n"], case["ham"], case["psi0"], stream_lbfgs=False))
    assert all(np.array_equal(a, b) for a, b in zip(between, fresh))
    assert np.array_equal(between[0], between[3])


def test_switch_and_refusals():
    import tensorrl_qas_amd as tq
    n = 14
    rng = np.random.default_rng(9)
    kind, q0, q1, pidx, th = random_gates(n, 10, rng)
    ham = random_hamiltonian(n, 6, rng)
    psi0 = random_state(n, rng)
    scale = lh.ham_scale(ham)
    circ = tq.Circuit(kind, q0, q1, pidx, th.size)
    e_ref = vo.energy_pauli(vo.run_circuit(psi0, kind, q0, q1, pidx, th), *ham)

    def refused(eng, code, call):
        with pytest.raises(tq.VQEError, match=rf"error {code}:"):
            call(eng)

    run = lambda e: e.minimize_lbfgs(th, maxiter=2)
    eng = _engine(n, ham, psi0, stream_lbfgs=False)
    eng.set_circuit(circ)
    refused(eng, EINVAL, run)                                   # the default handle
    eng.set_stream_grad()
    refused(eng, EINVAL, run)                                   # the gradient's switch is not this one
    eng.set_stream_grad(False)
    eng.set_stream_lbfgs(True)
    x, f, nfev, nit, st = run(eng)
    assert f < e_ref and nit >= 1
    refused(eng, EINVAL, lambda e: e.energy_grad(th))           # ... and this one is not the gradient's
    for setup, undo in ((lambda e: e.set_noise(0.01, 0.0, 1), lambda e: e.set_noise(0.0, 0.0, 1)),
                        (lambda e: e.set_shot_noise(0.1, 3), lambda e: e.set_shot_noise(0.0, 3)),
                        (lambda e: e.set_amplitude_shard(0, 2), lambda e: e.set_amplitude_shard(0, 1)),
                        (lambda e: e.set_term_shard(0, 2), lambda e: e.set_term_shard(0, 1))):
        setup(eng)
        refused(eng, ESTATE, run)
        eng.batch_load([circ], [th])
        refused(eng, ESTATE, lambda e: e.batch_run_minimize_lbfgs())
        refused(eng, ESTATE, lambda e: e.batch_run_env_step_lbfgs())
        undo(eng)
        assert abs(eng.energy(th) - e_ref) <= F_TOL * scale
    for bad in (dict(history=0), dict(history=17), dict(maxiter=-1), dict(maxfun=0), dict(max_ls=0), dict(gtol=-1e-3),
                dict(ftol=-1.0), dict(c1=0.0), dict(c1=1.0)):
        refused(eng, EINVAL, lambda e, bad=bad: e.minimize_lbfgs(th, **bad))
    assert abs(eng.energy(th) - e_ref) <= F_TOL * scale
    refused(eng, ESTATE, lambda e: e.batch_set_trace(True))     # no evaluation trace at n >= 14, as before
    x2, f2, *_ = run(eng)
    assert np.array_equal(x, x2) and f == f2
    eng.set_stream_lbfgs(False)
    refused(eng, EINVAL, run)
    assert abs(eng.energy(th) - e_ref) <= F_TOL * scale
    # n = 8: accepted, and no bit of the LDS kernel's run changes
    n8 = 8
    k8, a8, b8, p8, t8 = random_gates(n8, 20, rng)
    e8 = _engine(n8, random_hamiltonian(n8, 12, rng), random_state(n8, rng), stream_lbfgs=False)
    e8.set_circuit(tq.Circuit(k8, a8, b8, p8, t8.size))
    off = e8.minimize_lbfgs(t8, maxiter=4)
    e8.set_stream_lbfgs(True)
    on = e8.minimize_lbfgs(t8, maxiter=4)
    assert np.array_equal(off[0], on[0]) and off[1:] == on[1:]


def test_vec_env_lbfgs_at_14_qubits(tmp_path):
    """The 14-qubit chain of test_circuit_env_lbfgsb_at_14_qubits under VecCircuitEnv(device_optimizer="lbfgs"), which
    switches the streaming L-BFGS on for its engine: the native and the Python host loops agree, and every energy is
    the oracle's for that environment's circuit at its committed angles."""
    import torch
    from tensorrl_qas_amd import synthetic
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    n, B = 14, 2
    bound = float(3 * (n - 1) + n)
    conf = synthetic.write_chain_dataset(str(tmp_path / "dmrg-to-qc"), n, eigvals=[-bound, bound])
    conf["non_local_opt"]["global_iters"] = 20
    dev = torch.device("cuda:0")
    opts = dict(history=3, maxiter=6)
    vn = VecCircuitEnv(CircuitEnv, conf, dev, B, native=True, device_optimizer="lbfgs", lbfgs_opts=opts)
    vp = VecCircuitEnv(CircuitEnv, conf, dev, B, native=False, device_optimizer="lbfgs", lbfgs_opts=opts)
    assert vn.native and not vp.native and not vp.engine.device_info()["lds_path"]
    env = vp.envs[0]
    ham = (env.ham.xmask, env.ham.zmask, env.ham.coeff)
    psi0 = vo.statevector_from_qasm(open(env.spec.init_circuit_path()).read())
    table = env._actions_table
    nq = n * (n - 1)
    scripts = [[nq + 3 * 3 + 1, 5 * (n - 1) + 0], [2 * (n - 1) + 1, nq + 5 * 3 + 0]]      # RY q3, CNOT; CNOT, RX q5
    assert torch.equal(vn.reset(), vp.reset())
    for t in range(2):
        acts = [table[s[t]] for s in scripts]
        on, rn, dn = vn.step(acts)
        op, rp, dp = vp.step(acts)
        assert torch.equal(on, op) and torch.equal(rn, rp) and dn == dp, t
        for b in range(B):
            w, e = vn.envs[b], vp.envs[b]
            assert (w.energy, w.nfev) == (e.energy, e.nfev) and w.rwd == float(e.rwd)
            assert torch.equal(w.state, e.state)
            assert 1 <= e.nfev <= 20
            k, a, c, p, th = vo.ansatz_from_state(e.state.numpy(), n)
            e_ref = vo.energy_pauli(vo.run_circuit(psi0, k, a, c, p, th), *ham)
            assert abs(e.energy - e_ref) <= 1e-8, (t, b, e.energy, e_ref)
