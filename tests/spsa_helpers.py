"""numpy restatement of the device Adam-SPSA (tensorrl-qas_amd/csrc/spsa_m0.h, vqe_spsa.h), statement for
statement, and the oracle objectives it runs on in the tests.  A helper of tests/test_spsa_cpu.py and
tests/test_spsa_gpu.py, not a test.

    x = x0;  m = v = 0;  b1p = b2p = 1
    for k = 0 .. K-1:
        a_k = a / (k + 1 + stability)^alpha
        c_k = c / (k + 1)^gamma
        key = noise_key(seed, b, k)
        D_j = +1 if noise_uniform_k(key, j) < 0.5 else -1      (j = 0 .. P-1; D_hole = 0)
        f+ = E(x + c_k D)    evaluation 2k
        f- = E(x - c_k D)    evaluation 2k + 1
        g_j = (f+ - f-) / (2 c_k) * D_j
        b1k = beta_1 / (k + 1)^lamda
        m = b1k m + (1 - b1k) g
        v = beta_2 v + (1 - beta_2) g*g
        b1p *= b1k;  b2p *= beta_2
        x_j -= a_k * (m_j / (1 - b1p)) / (sqrt(v_j / (1 - b2p)) + eps)
    plain run: f = E(x_K), evaluation 2K, nfev = 2K + 1        (an environment step closes on the full circuit: the caller)
    K = 0 or no optimised parameter: that closing evaluation alone, evaluation 0, nfev = 1

The objective is ``fun(x, e)``: e is the evaluation's number inside the run (its id is eval_base + e).  The hash is
the engine's counter RNG as tests/qj_oracle.py restates it."""
import math

import numpy as np

import qj_oracle as qo

DEFAULTS = dict(maxiter=100, a=0.1, alpha=0.602, stability=0.0, c=0.1, gamma=0.101, beta_1=0.9, beta_2=0.999, lamda=0.0,
                eps=1e-8, seed=0)
FIELDS = ("maxiter", "a", "alpha", "stability", "c", "gamma", "beta_1", "beta_2", "lamda", "eps", "seed")


def options(**opts):
    o = dict(DEFAULTS)
    for k in opts:
        if k not in o:
            raise TypeError(k)
    o.update(opts)
    return o


def delta(seed, b, k, P, hole=-1):
    """The perturbation signs of iteration k for the circuit at position b of its batch"""
    key = qo.noise_key(int(seed), int(b), int(k))
    d = np.array([1.0 if qo.noise_uniform_k(key, j) < 0.5 else -1.0 for j in range(P)], np.float64)
    if hole >= 0:
        d[hole] = 0.0
    return d


def noise_gauss(seed, b, e):
    """The shot-noise draw of evaluation id e (vqe_device.h: noise_gauss)"""
    key = qo.noise_key(int(seed), int(b), int(e))
    u1 = qo.noise_uniform_k(key, 1 << 40)
    u2 = qo.noise_uniform_k(key, (1 << 40) + 1)
    return math.sqrt(-2.0 * math.log(1.0 - u1)) * math.cos(6.283185307179586 * u2)


class Result:
    """points[k] = x_k (k = 0 .. K); trials[e] = the point of evaluation e (2K of them, and the closing one of a plain
    run); values[e] its value; x = x_K; f = the closing value (None when fun is None); nfev as a plain run counts"""
    __slots__ = ("points", "trials", "values", "x", "f", "nfev", "K")


def spsa(fun, x0, hole=-1, b=0, feed=None, **opts):
    """Run the restatement from x0.  ``feed``: the values of the 2K trial evaluations (and, if longer, of the closing
    one) taken from a recording instead of ``fun`` - the teacher-forced form; ``fun`` may then be None."""
    o = options(**opts)
    x = np.array(x0, np.float64)
    P = x.size
    K = int(o["maxiter"]) if P - (hole >= 0) > 0 else 0
    m = np.zeros(P)
    v = np.zeros(P)
    b1p = b2p = 1.0
    r = Result()
    r.points, r.trials, r.values, r.K = [x.copy()], [], [], K

    def value(pt, e):
        if feed is not None and e < len(feed):
            return float(feed[e])
        return float(fun(pt, e))

    for k in range(K):
        a_k = o["a"] / (k + 1 + o["stability"]) ** o["alpha"]
        c_k = o["c"] / float(k + 1) ** o["gamma"]
        D = delta(o["seed"], b, k, P, hole)
        xp = x + c_k * D
        fp = value(xp, 2 * k)
        xm = x - c_k * D
        fm = value(xm, 2 * k + 1)
        g = (fp - fm) / (2.0 * c_k) * D
        b1k = o["beta_1"] / float(k + 1) ** o["lamda"]
        m = b1k * m + (1.0 - b1k) * g
        v = o["beta_2"] * v + (1.0 - o["beta_2"]) * g * g
        b1p *= b1k
        b2p *= o["beta_2"]
        x = x - a_k * (m / (1.0 - b1p)) / (np.sqrt(v / (1.0 - b2p)) + o["eps"])
        r.trials += [xp, xm]
        r.values += [fp, fm]
        r.points.append(x.copy())
    r.x = x
    r.f = None
    if fun is not None or (feed is not None and len(feed) > 2 * K):
        r.f = value(x, 2 * K)
        r.trials.append(x.copy())
        r.values.append(r.f)
    r.nfev = 2 * K + 1
    return r


# ---- oracle objectives --------------------------------------------------------------------------------------------
def oracle_objective(case, eval_base=0, b=0, noise=None):
    """fun(x, e) on the CPU oracle for a case dict(psi0, gates, ham): noiseless, or with ``noise`` =
    dict(seed, p1, p2, w1, w2, shot_sigma, shot_seed) one draw of the Pauli errors keyed by eval_base + e (the gate list
    then carries its noise gates) plus the shot term."""
    import lbfgs_helpers as lh
    if noise is None:
        return lambda x, e: lh.oracle_energy(case["psi0"], *case["gates"], x, case["ham"])
    import noise_pauli_oracle as npo

    def fun(x, e):
        eid = eval_base + e
        val = None
        if noise.get("p1", 0.0) > 0 or noise.get("p2", 0.0) > 0 or noise.get("w1") is not None or noise.get("w2") is not None:
            codes, _ = npo.draws(noise["seed"], b, eid, case["gates"][0], noise.get("w1"), noise.get("w2"),
                                 noise.get("p1", 0.0), noise.get("p2", 0.0))
            val = npo.energy(case["psi0"], case["gates"], np.asarray(x, np.float64), case["ham"], codes)
        else:
            val = lh.oracle_energy(case["psi0"], *case["gates"], x, case["ham"])
        if noise.get("shot_sigma", 0.0):
            val += noise["shot_sigma"] * noise_gauss(noise["shot_seed"], b, eid)
        return val

    return fun


# ---- the free-run cases of the GPU tests: lbfgs_helpers.trajectory_case(n, which, False), default options, seed 7,
# b = 0, K = 30 -------------------------------------------------------------------------------------------------------
FREE_CASES = [(4, 0), (4, 1), (6, 0), (6, 1), (8, 0), (8, 1)]
PRECONDITION_CASES = [(1, 0), (2, 0)] + FREE_CASES
FREE_OPTS = dict(maxiter=30, seed=7)
SENS_SIGMA = 1e-10          # the energy perturbation of the sensitivity measurement: N(0, 1e-10), the project's energy bound
_FREE = {}


def free_case(n, which):
    import lbfgs_helpers as lh
    return lh.trajectory_case(n, which, False)


def free_run(n, which):
    """-> (the restatement's run on oracle energies, its sensitivity): computed once per process.  The sensitivity is
    the largest deviation of any point x_k or trial point when every energy is off by N(0, 1e-10) - what a device
    energy within the project's bound of the oracle's may do to the points."""
    key = (n, which)
    if key not in _FREE:
        case = free_case(n, which)
        fun = oracle_objective(case)
        ref = spsa(fun, case["theta"], **FREE_OPTS)
        rng = np.random.default_rng(4321)
        off = spsa(lambda x, e: fun(x, e) + SENS_SIGMA * rng.normal(), case["theta"], **FREE_OPTS)
        sens = max(float(np.abs(p - q).max(initial=0.0)) for p, q in zip(ref.points + ref.trials, off.points + off.trials))
        _FREE[key] = (ref, sens)
    return _FREE[key]


def unpack_trace(tx, P, hole):
    """Rows of a device trace hold the optimised parameters only: put them back at their indices (the hole gets NaN)"""
    tx = np.asarray(tx)
    if hole < 0:
        return tx[:, :P].copy()
    out = np.full((tx.shape[0], P), np.nan)
    keep = [j for j in range(P) if j != hole]
    out[:, keep] = tx[:, :P - 1]
    return out
