"""Inputs and checks shared by tests/test_lds_sizes_gpu.py, tests/test_lds_placement_gpu.py and
tests/test_lds_placement_cpu.py: one set of inputs per register size N = 1 ... 13 of the LDS-resident kernels, the
oracle that goes with the size (numpy below 10 qubits, its C restatement from 10), the trace check of the device
COBYLA, and the walk over the optimiser's placement classes (vqe_cobyla_placement)."""
import functools

import numpy as np

import vqe_oracle as vo
from helpers import fermionic_hamiltonian, random_hamiltonian, random_state, tie_free_gates, with_noise_gates

SIZES = tuple(range(1, 14))          # LdsSizes of csrc/vqe_api.hip
E_TOL = 1e-10                        # energies (the project's bound)
A_TOL = 1e-12                        # amplitudes
X_TOL = 1e-9                         # trial points
P1, P2 = 0.25, 0.5                   # as test_noisy_env_step_optimises_pre_action_circuit: most evaluations draw errors
WIDE_MIN = 6                         # sizes with a WIDE instantiation of the minimiser
AFTER_SIMPLEX = 12                   # evaluations beyond the initial simplex the host replay must follow
CLASSES = ("resident", "staged", "global", "rows", "block")


# ---- oracle by size -------------------------------------------------------------------------------------------------
def run_circuit(n, psi0, kind, q0, q1, pidx, th, draws=None):
    if n >= 10:
        import c_oracle as co
        return co.run_circuit(n, psi0, kind, q0, q1, pidx, th, draws)
    return vo.run_circuit(psi0, kind, q0, q1, pidx, th, draws)


def energy_of(n, psi, ham):
    if n >= 10:
        import c_oracle as co
        return co.energy_pauli(n, psi, *ham)
    return vo.energy_pauli(psi, *ham)


def oracle_energy(n, psi0, gates, th, ham, draws=None):
    return energy_of(n, run_circuit(n, psi0, *gates, th, draws), ham)


# ---- inputs, one seed per N -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(n):
    """-> (psi0, ham): a random state and a complex-coefficient random Pauli sum; from 8 qubits (the unit path) a few
    terms of a number-conserving fermionic sum on top.  Terms with equal masks are merged."""
    rng = np.random.default_rng(7100 + n)
    psi0 = random_state(n, rng)
    terms = {}
    parts = [random_hamiltonian(n, 6 + 2 * n, rng, real=False)]
    if n >= 8:
        parts.append(fermionic_hamiltonian(n, n_hop=n, n_quad=n // 2, rng=rng, dressed=1))
    for xs, zs, cs in parts:
        for x, z, c in zip(xs, zs, cs):
            terms[(int(x), int(z))] = terms.get((int(x), int(z)), 0.0) + float(c)
    keys = sorted(terms)
    ham = (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint64),
           np.array([terms[k] for k in keys], np.float64))
    psi0.setflags(write=False)
    for a in ham:
        a.setflags(write=False)
    return psi0, ham


def engine(tq, n):
    psi0, ham = inputs(n)
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    return eng


def spread_rotations(n, P, rng, p_cnot=0.08):
    """P rotations for P > 3 n, where tie_free_gates runs out of (qubit, axis) pairs: qubits in turn, and never the
    axis of the previous rotation on the same qubit - two neighbouring rotations about one axis act as their sum, and
    the two equal simplex values that follow are a tie that the order of a sum decides."""
    kind, q0, q1, pidx = [], [], [], []
    last = [0] * n
    order = rng.permutation(n)
    for j in range(P):
        q = int(order[j % n])
        a = int(rng.choice([k for k in (1, 2, 3) if k != last[q]]))
        last[q] = a
        kind.append(a), q0.append(q), q1.append(-1), pidx.append(j)
        if rng.random() < p_cnot and n > 1:
            c = int(rng.integers(n))
            kind.append(0), q0.append(c), q1.append(int((c + 1 + rng.integers(n - 1)) % n)), pidx.append(-1)
    return tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)) + (rng.uniform(-np.pi, np.pi, P),)


def cobyla_circuit(n, P, seed, extra_rz=0):
    """A circuit of P rotations for the trajectory checks: on distinct (qubit, axis) pairs while there are enough of
    them (P <= 3 n: COBYLA then meets no exact ties), else spread_rotations.
    ``extra_rz``: that many more rotations WITHOUT a parameter of their own - RZ gates that share parameter 0 -, which
    lengthen the op list (the LDS carve-up) and leave the optimiser's problem size alone."""
    rng = np.random.default_rng(seed)
    kind, q0, q1, pidx, th = tie_free_gates(n, P, rng) if P <= 3 * n else spread_rotations(n, P, rng)
    if extra_rz:
        kind = np.concatenate([kind, np.full(extra_rz, 3, np.int32)])
        q0 = np.concatenate([q0, rng.integers(n, size=extra_rz).astype(np.int32)])
        q1 = np.concatenate([q1, np.full(extra_rz, -1, np.int32)])
        pidx = np.concatenate([pidx, np.zeros(extra_rz, np.int32)])
    return (kind, q0, q1, pidx), th


# ---- cases whose walk is decided by the algorithm, not by the last bit ----------------------------------------------
NOISE_SEED = 20240607
# (a marginal decision is flipped by one such draw in two to six - counted on the CPU at the decisions the criterion
# finds -, so 40 draws miss one with a probability below 0.1 %)
DECIDED_REPS = 40
DECIDED_TOL = X_TOL / 10


def default_maxfun(P):
    return P + 1 + AFTER_SIMPLEX + (8 if P <= 64 else 0)


def walk_is_decided(n, gates, x0, maxfun, noise=None, ham=None):
    """CPU only (the oracle and the library's host COBYLA; nothing of the device takes part).

    The device optimiser is cobyla_m0.h with another order of its own sums (tests/test_cobyla_emulation.py), so its
    internal quantities differ from the host's by rounding errors.  Where COBYLA compares two quantities that are
    equal, or nearly, in exact arithmetic - which vertex leaves the simplex, whether a step counts as an improvement -
    such an error decides, the two walks take different, equally valid branches and part by 0.01 ... 1 in ONE evaluation.
    That happens where the problem is over-parametrised (3 angles on one qubit, 25 on three) and where the objective
    jumps (Pauli errors); it says nothing about the kernel, and a case in which it happens inside the compared prefix
    cannot be compared at X_TOL (as a device L-BFGS case with a marginal decision cannot: lbfgs_helpers).

    The criterion, in the manner of lbfgs_helpers.gradient_sensitivity: the host COBYLA walks the oracle's objective
    once as it is and DECIDED_REPS times with every value off by a random error of the size of the evaluation's own
    rounding (2^-53 x gates x sum |c_k|).  The case is compared only if every trial point of the compared prefix
    (initial simplex + AFTER_SIMPLEX evaluations) stays within DECIDED_TOL, a tenth of X_TOL, in all of them."""
    import c_oracle as co
    import tensorrl_qas_amd as tq
    psi0 = inputs(n)[0]
    ham = inputs(n)[1] if ham is None else ham
    need = min(maxfun, x0.size + 1 + AFTER_SIMPLEX)
    eps = 2.0 ** -53 * gates[0].size * max(1.0, float(np.abs(ham[2]).sum()))

    seen = {}      # (the walks share the points of the initial simplex bit for bit)

    def walk(rng):
        opt = tq.HostCobyla(x0, 1.0, 1e-4, maxfun)
        xs = []
        for k in range(need):
            t = opt.ask()
            if t is None:
                break
            xs.append(t.copy())
            key = (k, t.tobytes())
            if key not in seen:
                dr = co.noise_draws(noise[0], noise[1], k + 1, gates[0], noise[2], noise[3]) if noise is not None else None
                seen[key] = co.energy_pauli(n, co.run_circuit(n, psi0, *gates, t, dr), *ham)
            opt.tell(seen[key] + (eps * rng.uniform(-1.0, 1.0) if rng is not None else 0.0))
        return xs

    ref = walk(None)
    for r in range(DECIDED_REPS):
        w = walk(np.random.default_rng(12345 + r))
        if len(w) != len(ref) or any(np.abs(a - b).max() > DECIDED_TOL for a, b in zip(ref, w)):
            return False
    return True


DISCARDED = []      # (label, j) of every case that did not take its base seed, for the reader of a test log


def first_decided(build, label, tries=40):
    """build(j) -> (case, (n, gates the optimiser sees, x0, maxfun, noise, ham)) for the j-th seed of a case; -> the case
    of the first j whose walk is decided (the recorded procedure of lbfgs_helpers.TRAJ_SEED, done on the spot: the
    case depends on sizes that only the placement query knows).  Every j > 0 is printed and kept in DISCARDED, and a
    case that would discard forty seeds fails: a size at which most seeds are rejected is to be noticed."""
    for j in range(tries):
        case, problem = build(j)
        if walk_is_decided(*problem):
            if j:
                DISCARDED.append((label, j))
                print(f"{label}: base seed and {j - 1} more had a marginal decision, seed number {j} is compared")
            return case
    raise AssertionError(f"{label}: no seed with a decided walk among {tries}")


@functools.lru_cache(maxsize=None)
def _cobyla_case(n, P, seed, noisy, extra_rz, maxfun, stream, ham_bytes):
    ham = None
    if ham_bytes is not None:
        ham = (np.frombuffer(ham_bytes[0], np.uint64), np.frombuffer(ham_bytes[1], np.uint64), np.frombuffer(ham_bytes[2], np.float64))

    def build(j):
        gates, th = cobyla_circuit(n, P, seed + 100000 * j, extra_rz)
        g = with_noise_gates(*gates) if noisy else gates
        noise = (NOISE_SEED, stream, P1, P2) if noisy else None
        return (gates, th), (n, g, th, maxfun or default_maxfun(P), noise, ham)
    return first_decided(build, f"cobyla_case(n={n}, P={P}, seed={seed}{', noisy' if noisy else ''}"
                                f"{f', +{extra_rz} ops' if extra_rz else ''}{', own Hamiltonian' if ham_bytes else ''})")


def cobyla_case(n, P, seed, noisy=False, extra_rz=0, maxfun=None, stream=0, ham=None):
    """cobyla_circuit(n, P, seed + 100000 j, extra_rz) for the first j = 0, 1, ... whose walk is decided for the run that
    will be compared: clean or with a channel behind every gate and the draws of (NOISE_SEED, stream), maxfun
    evaluations at most, the Hamiltonian of inputs(n) or ``ham``.  -> (gates WITHOUT channels, theta)"""
    key = None
    if ham is not None:      # (the cache key holds the arrays themselves)
        key = (np.ascontiguousarray(ham[0], np.uint64).tobytes(), np.ascontiguousarray(ham[1], np.uint64).tobytes(),
               np.ascontiguousarray(ham[2], np.float64).tobytes())
    return _cobyla_case(n, P, seed, bool(noisy), extra_rz, maxfun, stream, key)


# ---- the trace of the device COBYLA ---------------------------------------------------------------------------------
def check_trace(tq, n, gates, x0, ft, xt, nfev, maxfun, noise=None, ham=None):
    """Checks 3 / 4 of the size tests.  ``gates``: the circuit the optimiser sees (for an environment step the
    pre-action circuit), x0 its start, (ft, xt) the device's trace, nfev its evaluation count.
    * every traced value is the oracle's energy at the traced point - with ``noise`` = (seed, stream, p1, p2) under the
      oracle's draws of evaluation k + 1, numbered by gate position in THIS circuit (as the existing noisy tests);
    * the library's host COBYLA (bit-exact with scipy, tests/test_abi.py), told the device's values, proposes the same
      points (X_TOL) through the initial simplex and at least the next AFTER_SIMPLEX evaluations (the rule of
      test_device_cobyla_trajectory_many_parameters), or to the end of a shorter run.
    The second rule can only be asked of a case whose walk hangs on no marginal decision: see walk_is_decided."""
    psi0 = inputs(n)[0]
    ham = inputs(n)[1] if ham is None else ham
    P = x0.size
    assert 1 <= nfev <= maxfun
    assert np.array_equal(xt[0], x0)
    worst = 0.0
    for k in range(nfev):
        dr = None
        if noise is not None:
            import c_oracle as co
            seed, stream, p1, p2 = noise
            dr = co.noise_draws(seed, stream, k + 1, gates[0], p1, p2)
        e_ref = oracle_energy(n, psi0, gates, xt[k], ham, dr)
        worst = max(worst, abs(ft[k] - e_ref))
        assert abs(ft[k] - e_ref) < E_TOL, (n, P, k, ft[k], e_ref)
    opt = tq.HostCobyla(x0, 1.0, 1e-4, maxfun)
    agree = 0
    for k in range(nfev):
        t = opt.ask()
        if t is None or np.abs(t - xt[k]).max() > X_TOL:
            break
        opt.tell(ft[k])
        agree += 1
    need = min(nfev, P + 1 + AFTER_SIMPLEX)
    print(f"n={n} P={P}{' noisy' if noise else ''}: nfev {nfev}, worst |dE| {worst:.2e}, host replay in step for {agree}")
    assert agree >= need, (n, P, agree, need, nfev)
    return agree


def traced_minimize(eng, tq, circuits, maxfun, noise=None, new_gate=None):
    """circuits: [(gates, theta)].  One traced launch -> x, xraw, f, nfev, [(ft, xt) per circuit]."""
    if noise is not None:
        eng.set_noise(noise[2], noise[3], noise[0])          # evaluation counter starts at 0
    eng.batch_set_trace(True)
    eng.batch_load([tq.Circuit(*g, th.size) for g, th in circuits], [th for _, th in circuits])
    if new_gate is not None:
        eng.batch_set_new_gate(new_gate)
        eng.batch_run_env_step(1.0, 1e-4, maxfun)
    else:
        eng.batch_run_minimize(1.0, 1e-4, maxfun)
    x, f, nfev = eng.batch_fetch()
    xraw = eng.batch_fetch_xopt()
    traces = [eng.batch_fetch_trace(b, th.size) for b, (_, th) in enumerate(circuits)]
    eng.batch_set_trace(False)
    return x, xraw, f, nfev, traces


def minimize_and_check(eng, tq, n, gates, th, noisy):
    """Check 3 (clean) or 4 (noisy) on one circuit loaded alone (a case of cobyla_case with the same ``noisy``); the noisy
    run gets a channel behind every gate."""
    P = th.size
    maxfun = default_maxfun(P)
    noise = (NOISE_SEED, 0, P1, P2) if noisy else None
    g = with_noise_gates(*gates) if noisy else gates
    x, _, f, nfev, traces = traced_minimize(eng, tq, [(g, th)], maxfun, noise)
    ft, xt = traces[0]
    check_trace(tq, n, g, th, ft, xt, int(nfev[0]), maxfun, noise)
    # the result is one of the evaluations: its point, and the value the device had there (noisy: under that
    # evaluation's draws, which the trace check above has compared with the oracle)
    k = int(np.argmin([np.abs(xt[j] - x).max() for j in range(int(nfev[0]))]))
    assert np.abs(xt[k] - x).max() <= 1e-12 and float(f[0]) == ft[k], (n, P, k, float(f[0]), ft[k])
    if noisy and n > 1:      # most evaluations drew an error
        hit = sum(bool(np.any(_draws(noise, k + 1, g[0]))) for k in range(int(nfev[0])))
        assert hit > int(nfev[0]) // 2, (hit, nfev[0])
    if not noisy:
        psi0, ham = inputs(n)
        assert abs(oracle_energy(n, psi0, g, x, ham) - float(f[0])) < E_TOL


def _draws(noise, eval_id, kind):
    import c_oracle as co
    return co.noise_draws(noise[0], noise[1], eval_id, kind, noise[2], noise[3])


# ---- the placement classes ------------------------------------------------------------------------------------------
def class_runs(classify, p_values):
    """classify(P) -> hashable; -> [(first P, last P, class)] of the maximal runs over the ascending p_values"""
    runs = []
    for P in p_values:
        c = classify(P)
        if runs and runs[-1][2] == c:
            runs[-1][1] = P
        else:
            runs.append([P, P, c])
    return [tuple(r) for r in runs]


def boundaries(runs):
    """-> [(last P of a class, that class, first P of the next, that class)]"""
    return [(a[1], a[2], b[0], b[2]) for a, b in zip(runs, runs[1:])]


def round4(v):
    return (v + 3) & ~3


def single_circuit_sizes(gates, P):
    """(max_ops, max_pair, max_params) as vqe_batch_load rounds them for a batch of this one circuit"""
    kind = np.asarray(gates[0])
    ops = int(np.count_nonzero(kind != 0) + np.count_nonzero(kind == 5))
    pair = int(np.count_nonzero(np.isin(kind, (1, 2, 6, 7))))
    max_ops = round4(max(ops, 1))
    return max_ops, min(max_ops, round4(pair)), round4(max(P, 1))
