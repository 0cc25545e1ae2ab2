"""CPU: the numpy restatement of the device L-BFGS (tests/lbfgs_helpers.py) - the reference the GPU tests of
tests/test_lbfgs_gpu.py compare trajectories against - behaves as the algorithm says, and the cases those tests use
have no marginal decision (so a GPU divergence cannot hide behind a rounding excuse)."""
import numpy as np
import pytest

import lbfgs_helpers as lh
from helpers import random_gates, random_hamiltonian, random_state


def _quadratic(n, rng, cond=8.0):
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    a = q @ np.diag(np.linspace(1.0, cond, n)) @ q.T
    b = rng.normal(size=n)
    return (lambda x: (0.5 * float(x @ a @ x) - float(b @ x), a @ x - b)), np.linalg.solve(a, b)


def test_convex_quadratic_converges_to_gtol():
    rng = np.random.default_rng(1)
    fun, xstar = _quadratic(6, rng, cond=2.0)
    r = lh.lbfgs(fun, rng.normal(size=6), ftol=0.0)
    assert r.status == lh.GTOL
    assert np.abs(r.g).max() <= lh.DEFAULTS["gtol"]
    # n steps would do with exact line searches (the pairs then span the space); unit steps that merely pass the
    # Armijo test cost a few more
    assert r.nit <= 6 + 4, r.nit
    assert np.abs(r.x - xstar).max() <= 1e-5
    assert r.nfev == len(r.trials)
    fs = [t.f for t in r.trials if t.accepted is not False]
    assert all(b <= a for a, b in zip(fs, fs[1:]))          # Armijo: accepted values never increase


def test_final_energy_agrees_with_scipy_on_a_4_qubit_problem():
    from scipy.optimize import minimize
    n = 4
    rng = np.random.default_rng(11)
    kind, q0, q1, pidx, th = random_gates(n, 14, rng, p_cnot=0.3)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 12, rng)
    fun = lh.oracle_fun(psi0, kind, q0, q1, pidx, th.size, ham)
    scale = lh.ham_scale(ham)
    # the shift gradient is the derivative of the oracle energy
    f0, g0 = fun(th)
    h = 1e-6
    for j in range(th.size):
        tp, tm = th.copy(), th.copy()
        tp[j] += h
        tm[j] -= h
        assert abs(g0[j] - (fun(tp)[0] - fun(tm)[0]) / (2 * h)) < 1e-7 * scale
    assert abs(f0 - lh.oracle_energy(psi0, kind, q0, q1, pidx, th, ham)) <= 1e-12 * scale
    # Both are local searches and the landscape has several minima, so the common start lies inside one basin: a
    # minimum (found by scipy from the random angles), moved by 0.05 per angle.  A sanity check of the restatement, not
    # a trajectory match.
    opts = {"maxiter": 500, "ftol": 1e-15, "gtol": 1e-9}
    x0 = minimize(fun, th, jac=True, method="L-BFGS-B", options=opts).x + 0.05 * rng.normal(size=th.size)
    r = lh.lbfgs(fun, x0, scale=scale, maxiter=500, maxfun=5000, gtol=1e-9, ftol=1e-15)
    ref = minimize(fun, x0, jac=True, method="L-BFGS-B", options=opts)
    assert r.status in (lh.GTOL, lh.FTOL, lh.LINESEARCH) and r.f < fun(x0)[0]
    assert abs(r.f - ref.fun) <= 1e-8 * scale, (r.f, ref.fun, r.status, r.nit)


def test_uphill_gradient_is_status_2():
    calls = []

    def fun(x):
        calls.append(x.copy())
        return float(x @ x), -2.0 * x          # the negated gradient: every "descent" direction goes uphill

    x0 = np.array([1.0, -2.0, 0.5])
    r = lh.lbfgs(fun, x0)
    assert r.status == lh.LINESEARCH and r.nit == 0
    assert r.nfev == 1 + lh.DEFAULTS["max_ls"] == len(calls)
    assert np.array_equal(r.x, x0) and r.f == float(x0 @ x0)
    assert [t.t for t in r.trials[1:4]] == [1.0, 0.5, 0.25]
    assert all(t.accepted is False and t.slack < 0 for t in r.trials[1:])


@pytest.mark.parametrize("maxfun", [1, 2, 7])
def test_maxfun_is_status_3(maxfun):
    rng = np.random.default_rng(2)
    fun, _ = _quadratic(8, rng)
    r = lh.lbfgs(fun, rng.normal(size=8), maxfun=maxfun, gtol=0.0, ftol=0.0)
    assert r.status == lh.MAXFUN and r.nfev == maxfun == len(r.trials)
    assert r.f == min(t.f for t in r.trials if t.accepted is not False)


def test_maxiter_and_status_4():
    rng = np.random.default_rng(3)
    fun, _ = _quadratic(8, rng)
    x0 = rng.normal(size=8)
    r0 = lh.lbfgs(fun, x0, maxiter=0)
    assert r0.status == lh.MAXITER and r0.nit == 0 and r0.nfev == 1 and np.array_equal(r0.x, x0)
    r = lh.lbfgs(fun, x0, maxiter=3, gtol=0.0, ftol=0.0)
    assert r.status == lh.MAXITER and r.nit == 3


def test_history_eviction_at_m_2():
    rng = np.random.default_rng(4)
    fun, xstar = _quadratic(10, rng)
    x0 = rng.normal(size=10)
    r2 = lh.lbfgs(fun, x0, history=2, maxiter=8, gtol=0.0, ftol=0.0)
    assert r2.nit == 8 and r2.evictions == 6          # pairs 3..8 each push the oldest one out
    r9 = lh.lbfgs(fun, x0, history=9, maxiter=8, gtol=0.0, ftol=0.0)
    assert r9.evictions == 0
    # the first two iterations cannot tell the histories apart, the later ones can
    assert np.array_equal(r2.trials[1].x, r9.trials[1].x)
    assert not np.array_equal(r2.x, r9.x)
    assert r9.f <= r2.f


@pytest.mark.parametrize("key", lh.trajectory_cases(), ids=lambda k: f"n{k[0]}-h{k[1]}-{'su4' if k[2] else 'rot'}")
def test_gpu_trajectory_cases_have_no_marginal_decision(key):
    case = lh.trajectory_case(*key)
    r = lh.restated(("traj", key), case, **lh.TRAJ_OPTS)
    assert r.marginal == [], r.marginal
    assert r.nit >= 1 and r.nfev <= 1 + 6 * lh.DEFAULTS["max_ls"]
    # every accepted or rejected trial is decided by a slack well away from zero
    assert all(abs(t.slack) >= 1e-8 * case["scale"] for t in r.trials[1:])
    # and no trial point hangs on the last digits of a gradient (see gradient_sensitivity)
    sens = lh.gradient_sensitivity(case, r, **lh.TRAJ_OPTS)
    assert sens <= lh.X_SENSITIVITY_MAX, sens


def test_shared_and_unused_case_has_no_marginal_decision():
    case = lh.shared_unused_case()
    r = lh.restated("shared", case, **lh.TRAJ_OPTS)
    assert r.marginal == [], r.marginal
    assert r.x[2] == case["theta"][2] and r.nit >= 1          # the parameter no gate uses never moves
    assert lh.gradient_sensitivity(case, r, **lh.TRAJ_OPTS) <= lh.X_SENSITIVITY_MAX


def test_pre_action_circuit():
    kind = np.array([1, 0, 2, 3], np.int32)
    q0 = np.array([0, 0, 1, 1], np.int32)
    q1 = np.array([-1, 1, -1, -1], np.int32)
    pidx = np.array([0, -1, 1, 2], np.int32)
    th = np.array([0.1, 0.2, 0.3])
    (k, a, b, p), x0, hole = lh.pre_action(kind, q0, q1, pidx, th, 2)
    assert hole == 1 and list(k) == [1, 0, 3] and list(p) == [0, -1, 1] and list(x0) == [0.1, 0.3]
    (k, a, b, p), x0, hole = lh.pre_action(kind, q0, q1, pidx, th, 1)
    assert hole == -1 and list(k) == [1, 2, 3] and list(p) == [0, 1, 2] and list(x0) == list(th)
    assert lh.pre_action(kind, q0, q1, pidx, th, -1)[2] == -1


@pytest.mark.parametrize("n", [6, 12])
def test_gpu_env_step_cases_have_no_marginal_decision(n):
    for b in range(5):
        r, hole = lh.envstep_restated(n, b)
        assert r.marginal == [], (b, r.marginal)
        assert (hole >= 0) == (b < 3)
        assert lh.envstep_sensitivity(n, b) <= lh.X_SENSITIVITY_MAX, b


def test_gpu_trajectory_cases_cover_eviction():
    """history = 3, maxiter = 6: in every case the oldest pair leaves inside the compared run"""
    ev = {k: lh.restated(("traj", k), lh.trajectory_case(*k), **lh.TRAJ_OPTS).evictions for k in lh.trajectory_cases()}
    assert all(e > 0 for e in ev.values()), ev


def test_gpu_env_step_middle_case_has_no_marginal_decision():
    full, sub, hole = lh.envstep_middle_case()
    r = lh.restated("envstep-middle", sub, **lh.TRAJ_OPTS)
    assert r.marginal == [], r.marginal
    assert 0 < hole < full["theta"].size - 1 and r.nit >= 1
    assert lh.gradient_sensitivity(sub, r, **lh.TRAJ_OPTS) <= lh.X_SENSITIVITY_MAX


def test_gpu_trajectory_cases_hold_every_lds_size():
    """test_trajectory_parity (tests/test_lbfgs_gpu.py) runs k_lds_minimize_lbfgs at every compiled size of the LDS kernels"""
    assert sorted(lh.TRAJ_GATES) == list(range(1, 14))
