"""Cases and the CPU reference of the gradients of frozen Pauli-noise realisations (vqe_set_noise_grad); a
helper of tests/test_noise_grad_cpu.py and tests/test_noise_grad_gpu.py, not a test.  numpy only.

Reference: tests/noise_pauli_oracle.py (``draws``, ``energy``).  The gradient of ONE realisation is the parameter shift on
``energy`` with the realisation's codes held fixed: +-pi/2 per gate, summed over the gates that share a parameter.  Every
generator is a Pauli string, so the shift is exact.  RXX / RYY / RZZ are expanded into the oracle's gates by
tests/su4_helpers.py, each expanded gate carrying the code of the gate it came from (0 at every gate that is no noise
gate).  E_T and its gradient are the sums over t = 0 .. T-1 in ascending t, divided by T once."""
import numpy as np

import noise_pauli_oracle as npo
import su4_helpers as s4
from helpers import random_gates, random_hamiltonian, random_state, with_noise_gates

P1, P2 = 0.2, 0.3
G_LONG, G_SHORT = 70, 5
G_TOL = 1e-10


def scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


def realisation(psi0, gates, theta, ham, codes):
    """(E, dE/dtheta) of the circuit with the Pauli errors `codes` (one per gate of the list) inserted"""
    kind, q0, q1, pidx = (np.asarray(v) for v in gates)
    theta = np.asarray(theta, np.float64)
    k, a, b, p, src = s4.expand(kind, q0, q1, pidx, theta.size, with_source=True)
    dr = np.asarray(codes)[src]
    ext = s4.extend(theta)
    rot = [g for g in range(k.size) if 0 <= p[g] < theta.size]
    own = p.copy()                      # a private parameter per rotation gate behind the circuit's own and the two fixed angles
    for i, g in enumerate(rot):
        own[g] = ext.size + i
    base = np.concatenate([ext, [theta[p[g]] for g in rot]])
    e = npo.energy(psi0, (k, a, b, own), base, ham, dr)
    grad = np.zeros(theta.size)
    for i, g in enumerate(rot):
        tp, tm = base.copy(), base.copy()
        tp[ext.size + i] += np.pi / 2
        tm[ext.size + i] -= np.pi / 2
        grad[p[g]] += 0.5 * (npo.energy(psi0, (k, a, b, own), tp, ham, dr) - npo.energy(psi0, (k, a, b, own), tm, ham, dr))
    return e, grad


def codes_of(seed, b, base, T, kind, w1=None, w2=None, p=(P1, P2)):
    """the codes of the T realisations of batch position b and the smallest margin of a draw to a threshold"""
    out, margin = [], np.inf
    for t in range(T):
        c, m = npo.draws(seed, b, base + t, kind, w1, w2, *p)
        out.append(c)
        margin = min(margin, m)
    return out, margin


def mean(psi0, gates, theta, ham, codes, want_grad=True):
    """E_T (and its gradient) over the realisations `codes`, in ascending t"""
    e_sum, g_sum = 0.0, np.zeros(np.asarray(theta).size)
    for c in codes:
        if want_grad:
            e, g = realisation(psi0, gates, theta, ham, c)
            g_sum = g_sum + g
        else:
            e = energy(psi0, gates, theta, ham, c)
        e_sum = e_sum + e
    return e_sum / len(codes), g_sum / len(codes)


def energy(psi0, gates, theta, ham, codes):
    kind, q0, q1, pidx = (np.asarray(v) for v in gates)
    theta = np.asarray(theta, np.float64)
    k, a, b, p, src = s4.expand(kind, q0, q1, pidx, theta.size, with_source=True)
    return npo.energy(psi0, (k, a, b, p), s4.extend(theta), ham, np.asarray(codes)[src])


# ---- what the draws of the parity cases have to contain --------------------------------------------------------------------
def features(kind, q0, q1, codes):
    """of one realisation: {"none", "x_before_control", "y", "both"}"""
    kind, q0, q1, codes = (np.asarray(v) for v in (kind, q0, q1, codes))
    out = set()
    if not codes.any():
        out.add("none")
    for g in np.flatnonzero(codes):
        pa, pb = (int(codes[g]) & 3, int(codes[g]) >> 2) if kind[g] == npo.DEPOL2 else (int(codes[g]), 0)
        if pa == 2 or pb == 2:
            out.add("y")
        if pa and pb:
            out.add("both")
        flipped = {int(q0[g])} if pa in (1, 2) else set()
        if pb in (1, 2):
            flipped.add(int(q1[g]))
        if g + 1 < kind.size and kind[g + 1] == 0 and int(q0[g + 1]) in flipped:
            out.add("x_before_control")
    return out


# ---- the parity cases: n -> dict --------------------------------------------------------------------------------------------
PARITY_N = (3, 9, 10, 13)
PARITY_T = 3
PARITY_SEED = {3: 1103, 9: 1109, 10: 1110, 13: 1113}
_PARITY = {}


def parity_case(n):
    """n = 3, 9, 10: two circuits of 70 gates + their noise gates and one of 5 + 5 (a realisation WITHOUT an error of a
    70-gate circuit has probability < 0.8^70 ~ 1e-7: the short circuit is where one is found); n = 9 draws from all nine
    gate kinds.  n = 13: 2 distinct circuits at `batch` positions, more than the persistent grid has workgroups; the
    reference is computed at `check` positions only, the first and the last two.
    -> dict(psi0, ham, scale, circuits = [(gates, theta)], batch, check, seed)"""
    if n in _PARITY:
        return _PARITY[n]
    rng = np.random.default_rng(800 + n)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 10, rng)

    def circuit(G):
        kind, q0, q1, pidx, th = (s4.random_gates_su4(n, G, rng) if n == 9 else random_gates(n, G, rng, p_cnot=0.4))
        return with_noise_gates(kind, q0, q1, pidx), th

    if n == 13:
        distinct = [circuit(G_LONG), circuit(G_LONG)]
        batch = 260
        circuits = [distinct[b & 1] for b in range(batch)]
        check = [0, batch - 2, batch - 1]
    else:
        circuits = [circuit(G_LONG), circuit(G_SHORT), circuit(G_LONG)]
        batch, check = 3, [0, 1, 2]
    _PARITY[n] = {"n": n, "psi0": psi0, "ham": ham, "scale": scale(ham), "circuits": circuits, "batch": batch, "check": check,
                  "seed": PARITY_SEED[n]}
    return _PARITY[n]


def parity_codes(case, base=0, T=PARITY_T, w1=None, w2=None):
    """{b: [codes of realisation t]} of the checked positions, and the margin"""
    out, margin = {}, np.inf
    for b in case["check"]:
        out[b], m = codes_of(case["seed"], b, base, T, case["circuits"][b][0][0], w1, w2)
        margin = min(margin, m)
    return out, margin


def parity_features():
    """the union over every checked realisation of every parity case"""
    seen = set()
    for n in PARITY_N:
        case = parity_case(n)
        codes, _ = parity_codes(case)
        for b, per_t in codes.items():
            kind, q0, q1, _ = case["circuits"][b][0]
            for c in per_t:
                seen |= features(kind, q0, q1, c)
    return seen


_REF = {}


def parity_reference(n):
    """{b: (E_T, grad)} of parity_case(n), computed once per process"""
    if n not in _REF:
        case = parity_case(n)
        codes, _ = parity_codes(case)
        _REF[n] = {b: mean(case["psi0"], case["circuits"][b][0], case["circuits"][b][1], case["ham"], codes[b]) for b in case["check"]}
    return _REF[n]


# ---- the statistics case: n = 3, one circuit at 64 positions, T = 64 ----------------------------------------------------------
STAT_B, STAT_T, STAT_SEED = 64, 64, 20260
_STAT = {}


def stat_case():
    if "case" not in _STAT:
        n = 3
        rng = np.random.default_rng(4100)
        psi0, ham = random_state(n, rng), random_hamiltonian(n, 8, rng)
        kind, q0, q1, pidx, th = random_gates(n, 8, rng, p_cnot=0.4)
        _STAT["case"] = {"n": n, "psi0": psi0, "ham": ham, "gates": with_noise_gates(kind, q0, q1, pidx), "theta": th,
                         "seed": STAT_SEED, "p": (0.05, 0.08)}
    return _STAT["case"]


def stat_exact_grad(c):
    """the gradient of tr(rho H) under the depolarising channels (density-matrix oracle, parameter shift gate by gate)"""
    import vqe_oracle as vo
    kind, q0, q1, pidx = c["gates"]
    th = c["theta"]
    rot = [g for g in range(kind.size) if pidx[g] >= 0]
    own = np.full(kind.size, -1, np.int32)
    own[rot] = np.arange(len(rot))
    base = np.array([th[pidx[g]] for g in rot])
    run = lambda t: vo.energy_dm(vo.run_circuit_dm(c["psi0"], kind, q0, q1, own, t, *c["p"]), *c["ham"])
    grad = np.zeros(th.size)
    for i, g in enumerate(rot):
        tp, tm = base.copy(), base.copy()
        tp[i] += np.pi / 2
        tm[i] -= np.pi / 2
        grad[pidx[g]] += 0.5 * (run(tp) - run(tm))
    return grad


def stat_oracle_blocks(c):
    """(STAT_B, P): the block means of the sampled gradient as the CPU oracle computes them"""
    if "blocks" not in _STAT:
        rows, memo = [], {}
        for b in range(STAT_B):
            codes, _ = codes_of(c["seed"], b, 0, STAT_T, c["gates"][0], p=c["p"])
            g_sum = np.zeros(c["theta"].size)
            for cd in codes:                      # (ascending t; equal code lists have equal gradients)
                key = tuple(int(v) for v in cd)
                if key not in memo:
                    memo[key] = realisation(c["psi0"], c["gates"], c["theta"], c["ham"], cd)[1]
                g_sum = g_sum + memo[key]
            rows.append(g_sum / STAT_T)
        _STAT["blocks"] = np.array(rows)
    return _STAT["blocks"]


def within_4_sigma(blocks, exact):
    """every entry of the mean of the block means within 4 standard errors of the exact gradient -> (ok, mean, sigma)"""
    m = blocks.mean(axis=0)
    s = blocks.std(axis=0, ddof=1) / np.sqrt(blocks.shape[0])
    return bool(np.all(np.abs(m - exact) <= 4 * s)), m, s
