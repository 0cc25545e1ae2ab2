"""numpy restatement of the device L-BFGS (tensorrl-qas_amd/csrc/vqe_lbfgs.h), decision for decision, and
the oracle objective it runs on in the tests: energies from vqe_oracle, gradients by the exact parameter shift.

The algorithm (the issue's, with the details it leaves open fixed as the kernel fixes them):

    (f, g) = eval(x0); nfev = 1; nit = 0
    loop:
        nit == maxiter                 -> status 4          (so maxiter = 0 returns x0)
        max|g_j| <= gtol               -> status 0
        nfev >= maxfun                 -> status 3          (no evaluation left for a line search)
        d = -H g: two-loop recursion over the stored pairs, newest first, H0 = (s.y)/(y.y) of the newest pair;
            no pair stored: d = -g / max(1, |g|_2)
        dg = g.d; dg >= 0: drop the history, take the no-pair direction
        t = 1; up to max_ls trials:
            (ft, gt) = eval(x + t d); nfev += 1
            ft <= f + c1 t dg          -> accept
            else nfev == maxfun        -> status 3
            else t *= 0.5
        no trial accepted              -> status 2 (x, f unchanged)
        s = t d, y = gt - g; stored iff s.y > 1e-10 y.y (the oldest pair leaves when m are held)
        converged = f - ft <= ftol max(|f|, |ft|, 1)
        x, f, g = x + t d, ft, gt; nit += 1
        converged                      -> status 1

A decision is *marginal* when rounding could turn it: an Armijo test with |slack| < 1e-8 scale, or a stop / store test
whose two sides are within a factor 2 of each other.  The GPU trajectory tests only use cases without one.
"""
import numpy as np

import su4_helpers as s4
import vqe_oracle as vo

GTOL, FTOL, LINESEARCH, MAXFUN, MAXITER = range(5)
DEFAULTS = dict(history=8, maxiter=100, maxfun=1000, max_ls=20, gtol=1e-6, ftol=1e-12, c1=1e-4)


class Trial:
    """One evaluation: the point, its value, whether the Armijo test took it (None: the evaluation of x0), the slack
    f + c1 t dg - ft of that test."""
    __slots__ = ("x", "f", "accepted", "slack", "t")

    def __init__(self, x, f, accepted, slack, t):
        self.x, self.f, self.accepted, self.slack, self.t = x, f, accepted, slack, t


class Result:
    __slots__ = ("x", "f", "g", "nfev", "nit", "status", "trials", "marginal", "evictions")

    def __iter__(self):
        return iter((self.x, self.f, self.nfev, self.nit, self.status))


def _within2(a, b):
    """a and b (both >= 0) within a factor 2 of each other"""
    return 0.5 * b <= a <= 2.0 * b and (a > 0 or b > 0)


def lbfgs(fun, x0, scale=1.0, **opts):
    """Minimise ``fun(x) -> (f, g)`` from x0.  Returns a Result: x, f, g, nfev, nit, status, the list of Trials, the
    list of marginal decisions (strings, empty when every decision is robust) and the number of evicted pairs."""
    o = dict(DEFAULTS)
    o.update(opts)
    m, maxiter, maxfun, max_ls = int(o["history"]), int(o["maxiter"]), int(o["maxfun"]), int(o["max_ls"])
    gtol, ftol, c1 = float(o["gtol"]), float(o["ftol"]), float(o["c1"])
    r = Result()
    r.trials, r.marginal, r.evictions = [], [], 0
    x = np.array(x0, np.float64)
    f, g = fun(x)
    g = np.array(g, np.float64)
    nfev, nit = 1, 0
    r.trials.append(Trial(x.copy(), f, None, 0.0, 0.0))
    pairs = []                                   # (s, y, s.y, y.y), oldest first
    while True:
        if nit == maxiter:
            status = MAXITER
            break
        gmax = float(np.abs(g).max(initial=0.0))
        if gtol > 0 and _within2(gmax, gtol):
            r.marginal.append(f"gtol test at nit {nit}: max|g| = {gmax:.3e}")
        if gmax <= gtol:
            status = GTOL
            break
        if nfev >= maxfun:
            status = MAXFUN
            break

        def steepest():
            return -g / max(1.0, float(np.sqrt(np.dot(g, g))))

        if pairs:
            q = g.copy()
            alpha = []
            for s, y, sy, yy in reversed(pairs):
                a = float(np.dot(s, q)) / sy
                alpha.append(a)
                q -= a * y
            q *= pairs[-1][2] / pairs[-1][3]
            for (s, y, sy, yy), a in zip(pairs, reversed(alpha)):
                beta = float(np.dot(y, q)) / sy
                q += (a - beta) * s
            d = -q
            dg = float(np.dot(g, d))
            if abs(dg) < 1e-12 * scale:
                r.marginal.append(f"descent test at nit {nit}: g.d = {dg:.3e}")
            if dg >= 0.0:
                pairs = []
                d = steepest()
                dg = float(np.dot(g, d))
        else:
            d = steepest()
            dg = float(np.dot(g, d))
        t, accepted = 1.0, False
        for _ in range(max_ls):
            xt = x + t * d
            ft, gt = fun(xt)
            gt = np.array(gt, np.float64)
            nfev += 1
            slack = f + c1 * t * dg - ft
            accepted = ft <= f + c1 * t * dg
            r.trials.append(Trial(xt.copy(), ft, bool(accepted), slack, t))
            if abs(slack) < 1e-8 * scale:
                r.marginal.append(f"Armijo test at evaluation {nfev}: slack = {slack:.3e}")
            if accepted:
                break
            if nfev == maxfun:
                break
            t *= 0.5
        if not accepted:
            status = MAXFUN if nfev == maxfun else LINESEARCH      # (the maxfun test comes before the count of trials)
            break
        s, y = t * d, gt - g
        sy, yy = float(np.dot(s, y)), float(np.dot(y, y))
        if _within2(abs(sy), 1e-10 * yy):
            r.marginal.append(f"pair test at nit {nit}: s.y = {sy:.3e}, y.y = {yy:.3e}")
        if sy > 1e-10 * yy:
            if len(pairs) == m:
                pairs.pop(0)
                r.evictions += 1
            pairs.append((s, y, sy, yy))
        conv = ftol * max(abs(f), abs(ft), 1.0)
        if conv > 0 and _within2(abs(f - ft), conv):
            r.marginal.append(f"ftol test at nit {nit}: f - ft = {f - ft:.3e}")
        converged = (f - ft) <= conv
        x, f, g = xt, ft, gt
        nit += 1
        if converged:
            status = FTOL
            break
    r.x, r.f, r.g, r.nfev, r.nit, r.status = x, f, g, nfev, nit, status
    return r


# ---- the oracle objective -----------------------------------------------------------------------------------------
def oracle_fun(psi0, kind, q0, q1, pidx, n_params, ham):
    """x -> (E(x), dE/dx) on the CPU oracle (its C restatement c_oracle, which tests/test_oracle.py pins to
    vqe_oracle: a gradient is two energies per rotation gate, and numpy takes seconds for one at 12 qubits).
    RXX / RYY / RZZ are expanded by su4_helpers.  Gradient: the exact parameter shift gate by gate, as _shift_grad of
    test_grad_gpu.py - the gate is shifted by +-pi/2 on the state in front of it and the rest of the circuit follows,
    so a shared parameter is shifted one gate at a time."""
    import c_oracle as co
    k, a, b, p = s4.expand(kind, q0, q1, pidx, n_params)
    rot = [g for g in range(k.size) if 0 <= p[g] < n_params]
    one = np.zeros(1, np.int32)
    n = int(np.log2(np.asarray(psi0).size))
    run = lambda psi, lo, hi, pp, th: co.run_circuit(n, psi, k[lo:hi], a[lo:hi], b[lo:hi], pp, th)

    def fun(x):
        th = s4.extend(x)
        grad = np.zeros(n_params)
        psi, at = np.asarray(psi0, np.complex128), 0
        for g in rot:
            psi = run(psi, at, g, p[at:g], th)
            at = g
            for sg in (1.0, -1.0):
                shifted = run(psi, g, g + 1, one, np.array([th[p[g]] + sg * np.pi / 2]))
                end = run(shifted, g + 1, k.size, p[g + 1:], th)
                grad[p[g]] += sg * 0.5 * co.energy_pauli(n, end, *ham)
        psi = run(psi, at, k.size, p[at:], th)
        return co.energy_pauli(n, psi, *ham), grad

    return fun


def oracle_energy(psi0, kind, q0, q1, pidx, x, ham):
    return s4.energy(psi0, kind, q0, q1, pidx, np.asarray(x, np.float64), ham)


def ham_scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


# ---- the cases of the GPU trajectory tests (tests/test_lbfgs_gpu.py); tests/test_lbfgs_cpu.py checks on the CPU that
# none of them has a marginal decision --------------------------------------------------------------------------------
TRAJ_GATES = {1: 6, 2: 10, 3: 16, 4: 20, 5: 24, 6: 30, 7: 32, 8: 34, 9: 36, 10: 40, 11: 38, 12: 36, 13: 24}
TRAJ_OPTS = dict(history=3, maxiter=6, maxfun=200)
# (n, which, su4) -> seed, where the default 500 + n had a marginal decision (n = 1) or trial points that hang on the
# last digits of the gradient (gradient_sensitivity: the flat landscapes of the fermionic Hamiltonian and of 13
# qubits, where the first quasi-Newton steps are tens of radians long).  Taken from 500 + n + 100 j: the first seed
# that passes tests/test_lbfgs_cpu.py with room to spare and still evicts a pair inside the run.
TRAJ_SEED = {(1, 0, False): 509, (6, 1, False): 1006, (6, 1, True): 706, (10, 1, False): 2510, (12, 1, False): 812,
             (12, 1, True): 712, (13, 0, False): 1113, (13, 1, False): 1513,
             # the sizes added for tests/test_lds_sizes_gpu.py, by the same procedure (room to spare: a sensitivity of at
             # most half of X_SENSITIVITY_MAX)
             (5, 1, False): 905, (8, 1, False): 608, (9, 1, False): 609, (11, 1, False): 1411}


def trajectory_cases():
    """(n, which Hamiltonian, su4) of every trajectory case"""
    out = []
    for n in sorted(TRAJ_GATES):
        for which in range(2 if n >= 4 else 1):
            out.append((n, which, False))
            if n in (6, 12):
                out.append((n, which, True))
    return out


def trajectory_case(n, which, su4):
    """-> dict(psi0, gates = (kind, q0, q1, pidx), theta, ham, scale)"""
    from helpers import fermionic_hamiltonian, random_gates, random_hamiltonian, random_state
    rng = np.random.default_rng(TRAJ_SEED.get((n, which, su4), 500 + n))
    G = TRAJ_GATES[n]
    if su4:
        kind, q0, q1, pidx, th = s4.random_gates_su4(n, G, rng, p_cnot=0.3, p_two=0.3)
    else:
        kind, q0, q1, pidx, th = random_gates(n, G, rng, p_cnot=0.3 if n > 1 else 0.0)
    psi0 = random_state(n, rng)
    hams = [random_hamiltonian(n, 6 + 2 * n, rng, real=False)]
    if n >= 4:
        hams.append(fermionic_hamiltonian(n, n_hop=n, n_quad=n // 2, rng=rng, dressed=1))
    ham = hams[which]
    return dict(n=n, psi0=psi0, gates=(kind, q0, q1, pidx), theta=th, ham=ham, scale=ham_scale(ham))


def shared_unused_case():
    """The 5-qubit circuit of test_grad_shared_and_unused_parameters (tests/test_grad_gpu.py): parameter 0 drives an RY
    on q1 and an RX on q3, parameter 2 drives no gate."""
    from helpers import random_hamiltonian, random_state
    n = 5
    rng = np.random.default_rng(7)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 20, rng, real=False)
    kind = np.array([2, 0, 1, 3, 0, 2], np.int32)
    q0 = np.array([1, 1, 3, 0, 3, 4], np.int32)
    q1 = np.array([-1, 2, -1, -1, 0, -1], np.int32)
    pidx = np.array([0, -1, 0, 1, -1, 3], np.int32)
    return dict(n=n, psi0=psi0, gates=(kind, q0, q1, pidx), theta=np.array([0.7, -1.1, 2.0, 0.4]), ham=ham,
                scale=ham_scale(ham))


def pre_action(kind, q0, q1, pidx, theta, new_gate):
    """The circuit the optimiser sees in an environment step: without gate ``new_gate`` (-1: none); if that gate is a
    rotation its parameter (the hole) is no variable and the indices above it move down.
    -> ((kind, q0, q1, pidx), x0, hole)"""
    if new_gate < 0:
        return (kind, q0, q1, pidx), np.array(theta, np.float64), -1
    hole = int(pidx[new_gate])
    keep = np.arange(kind.size) != new_gate
    p2 = pidx[keep].copy()
    if hole >= 0:
        p2[p2 > hole] -= 1
    x0 = np.array([t for j, t in enumerate(theta) if j != hole], np.float64)
    return (kind[keep], q0[keep], q1[keep], p2), x0, hole


ENVSTEP_SEED = {}       # n -> seed, where the default 700 + n had a marginal decision


def envstep_case(n):
    """Five circuits of an environment-step batch: the new gate is the last rotation (circuits 0..2), a CNOT
    (circuit 3), none (circuit 4).  -> dict(psi0, ham, scale, circuits = [dict(gates, theta, new_gate)])"""
    from helpers import random_gates, random_hamiltonian, random_state
    rng = np.random.default_rng(ENVSTEP_SEED.get(n, 700 + n))
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 6 + 2 * n, rng, real=False)
    circuits = []
    for b in range(5):
        kind, q0, q1, pidx, th = random_gates(n, 12 + 3 * b, rng, p_cnot=0.3)
        if b < 3:
            ng = int(np.nonzero(kind != 0)[0][-1])
        elif b == 3:
            ng = int(np.nonzero(kind == 0)[0][0])
        else:
            ng = -1
        circuits.append(dict(gates=(kind, q0, q1, pidx), theta=th, new_gate=ng))
    return dict(n=n, psi0=psi0, ham=ham, scale=ham_scale(ham), circuits=circuits)


def _envstep_pre_action(n, b):
    case = envstep_case(n)
    c = case["circuits"][b]
    gates, x0, hole = pre_action(*c["gates"], c["theta"], c["new_gate"])
    return dict(psi0=case["psi0"], gates=gates, theta=x0, ham=case["ham"], scale=case["scale"]), hole


def envstep_restated(n, b):
    """The restatement's run on the pre-action circuit of circuit b of envstep_case(n) -> (Result, hole)"""
    sub, hole = _envstep_pre_action(n, b)
    return restated(("envstep", n, b), sub, **TRAJ_OPTS), hole


def envstep_sensitivity(n, b):
    """gradient_sensitivity of that run"""
    sub, _ = _envstep_pre_action(n, b)
    return gradient_sensitivity(sub, envstep_restated(n, b)[0], **TRAJ_OPTS)


def envstep_middle_case():
    """An environment step whose new gate is a rotation in the middle of the circuit, so that its parameter (the hole)
    has variables on both sides: circuit 4 of envstep_case(6) with the rotation nearest to the middle as the new gate.
    -> (dict(psi0, ham, scale, gates, theta, new_gate), the pre-action case for restated(), hole)"""
    case = envstep_case(6)
    c = case["circuits"][4]
    kind, pidx = c["gates"][0], c["gates"][3]
    rot = np.nonzero(kind != 0)[0]
    ng = int(rot[rot.size // 2])
    gates, x0, hole = pre_action(*c["gates"], c["theta"], ng)
    assert 0 < hole < c["theta"].size - 1 and hole == int(pidx[ng])
    full = dict(psi0=case["psi0"], ham=case["ham"], scale=case["scale"], gates=c["gates"], theta=c["theta"], new_gate=ng)
    sub = dict(psi0=case["psi0"], gates=gates, theta=x0, ham=case["ham"], scale=case["scale"])
    return full, sub, hole


_RESTATED = {}


def restated(key, case, **opts):
    """The restatement's run on a case, computed once per process and shared by the tests that compare against it."""
    if key not in _RESTATED:
        fun = oracle_fun(case["psi0"], *case["gates"], case["theta"].size, case["ham"])
        _RESTATED[key] = lbfgs(fun, case["theta"], scale=case["scale"], **opts)
    return _RESTATED[key]


X_TOL = 1e-9                # the bound of the GPU tests on every trial point
X_SENSITIVITY_MAX = 1e-10   # a tenth of it: what gradient_sensitivity may return for a case that is compared


def gradient_sensitivity(case, ref, **opts):
    """How far the trial points move when every gradient component is off by a rounding error.

    No decision of a run may be marginal and its points may still not be comparable at X_TOL: a quasi-Newton step
    multiplies an error of the gradient by the inverse-Hessian estimate, which on a flat stretch of the landscape
    (small y) is in the hundreds (steps of tens of radians), and each later step builds on the moved point.  The
    device gradient and the shift gradient are two different roundings of the same number: every gate application
    rounds the state once (2^-53 relative) and the energy weighs it with sum |c_k| = scale, so they differ by about
    2^-53 * gates * scale per component.  A case is compared only if a random error of that size in every gradient
    leaves every trial point within X_SENSITIVITY_MAX, a tenth of the bound the GPU test sets.

    -> max over the trial points of |x_perturbed - x|, inf when the perturbed run takes another number of trials"""
    eps = 2.0 ** -53 * case["gates"][0].size * case["scale"]
    fun = oracle_fun(case["psi0"], *case["gates"], case["theta"].size, case["ham"])
    rng = np.random.default_rng(12345)

    def off(x):
        f, g = fun(x)
        return f, g + eps * rng.uniform(-1.0, 1.0, g.size)

    r = lbfgs(off, case["theta"], scale=case["scale"], **opts)
    if len(r.trials) != len(ref.trials):
        return np.inf
    return max(float(np.abs(a.x - b.x).max(initial=0.0)) for a, b in zip(ref.trials, r.trials))
