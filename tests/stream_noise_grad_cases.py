"""Cases of the gradients of frozen Pauli-noise realisations on the streaming path (vqe_set_stream_noise_grad, DESIGN
4.21); a helper of tests/test_stream_noise_grad_cpu.py and tests/test_stream_noise_grad_gpu.py, not a test.  numpy only.

Reference: tests/noise_grad_cases.py as it stands (``codes_of``, ``realisation``, ``mean``, ``features``): the draws and
the energy of tests/noise_pauli_oracle.py, the exact parameter shift with the realisation's codes held fixed.
Shapes: at most 13 gates + their noise gates per circuit, 10 Pauli terms, T = 3 - the oracle then computes a few hundred
energies at 2^14 .. 2^16 amplitudes.  A circuit of 3 + 3 gates sits in every batch: with p = (0.2, 0.3) a realisation
without an error is rare in the longer ones."""
import numpy as np

import noise_grad_cases as ngc
import noise_pauli_oracle as npo
import qj_oracle as qo
import su4_helpers as s4
from helpers import random_gates, random_hamiltonian, random_state, with_noise_gates

P = (ngc.P1, ngc.P2)            # (0.2, 0.3)
T = 3
G_LONG, G_SHORT = 13, 3
K_BACK = 3                      # kGradOpsPerSweep of csrc/vqe_stream_grad.h: ops per backward sweep
PARITY_N = (14, 15, 16)
# rng seed of the circuits, noise seed: chosen so that test_stream_noise_grad_cpu.py's preconditions hold
PARITY_SEED = {14: (1400, 2174), 15: (1501, 2115), 16: (1600, 2116)}
MAX_RESIDENT_16 = 2             # < B T = 6: three chunks
_CASE, _REF = {}, {}


def records(kind, codes):
    """the compiled op list of one realisation as k_s_compile writes it: "r" for a rotation, "z" for the OP_PZ record of
    a drawn Z or Y (one per qubit of the noise gate that carries one); CNOTs and X errors leave no op"""
    out = []
    for k, c in zip(np.asarray(kind), np.asarray(codes)):
        k, c = int(k), int(c)
        if k in (1, 2, 3, 6, 7, 8):
            out.append("r")
        elif k == 4 and c in (2, 3):
            out.append("z")
        elif k == 5:
            out += ["z"] * (int((c & 3) in (2, 3)) + int((c >> 2) in (2, 3)))
    return out


def parity_case(n):
    """n = 14: three circuits (13 + 13, 3 + 3, 13 + 13 gates); 15: the same from all nine gate kinds; 16: ONE circuit of
    13 + 13 gates at two batch positions.  -> dict(n, psi0, ham, scale, circuits = [(gates, theta)], seed)"""
    if n in _CASE:
        return _CASE[n]
    rs, seed = PARITY_SEED[n]
    rng = np.random.default_rng(rs)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 10, rng)

    def circuit(G):
        kind, q0, q1, pidx, th = (s4.random_gates_su4(n, G, rng) if n == 15 else random_gates(n, G, rng, p_cnot=0.4))
        return with_noise_gates(kind, q0, q1, pidx), th

    if n == 16:
        one = circuit(G_LONG)
        circuits = [one, one]
    else:
        circuits = [circuit(G_LONG), circuit(G_SHORT), circuit(G_LONG)]
    _CASE[n] = {"n": n, "psi0": psi0, "ham": ham, "scale": ngc.scale(ham), "circuits": circuits, "seed": seed}
    return _CASE[n]


def depol_margin(seed, b, e, kinds, p=P):
    """the smallest distance of a draw of (stream b, evaluation e) to a threshold of its depolarising slot: p itself and
    the code boundaries k p / m below it (noise_pauli_oracle.draws reports the margins of table slots only)"""
    key, margin = qo.noise_key(seed, b, e), np.inf
    for g, k in enumerate(kinds):
        if int(k) in (npo.DEPOL1, npo.DEPOL2):
            pk, m = (p[0], 3) if int(k) == npo.DEPOL1 else (p[1], 15)
            u = qo.noise_uniform_k(key, g)
            margin = min([margin] + [abs(u - pk * j / m) for j in range(1, m + 1)])
    return margin


def parity_codes(case, base=0, t_real=T, w1=None, w2=None, p=P, seed=None):
    """{b: [codes of realisation t]} and the smallest margin of a draw to its threshold (seed: the case's unless given)"""
    out, margin = {}, np.inf
    seed = case["seed"] if seed is None else seed
    for b, (gates, _) in enumerate(case["circuits"]):
        out[b], m = ngc.codes_of(seed, b, base, t_real, gates[0], w1, w2, p)
        margin = min(margin, m)
        if w1 is None and w2 is None:
            margin = min([margin] + [depol_margin(seed, b, base + t, gates[0], p) for t in range(t_real)])
    return out, margin


def parity_reference(n):
    """{b: (E_T, grad)} of parity_case(n), computed once per process"""
    if n not in _REF:
        case = parity_case(n)
        codes, _ = parity_codes(case)
        _REF[n] = {b: ngc.mean(case["psi0"], g, th, case["ham"], codes[b]) for b, (g, th) in enumerate(case["circuits"])}
    return _REF[n]


def preconditions():
    """what the draws of the parity cases contain, from the draws alone:
    -> (features seen, positions o % 3 of an OP_PZ record, a circuit whose realisations differ in op count, margin)"""
    seen, pos, differ, margin = set(), set(), False, np.inf
    for n in PARITY_N:
        case = parity_case(n)
        codes, m = parity_codes(case)
        margin = min(margin, m)
        for b, per_t in codes.items():
            kind, q0, q1, _ = case["circuits"][b][0]
            counts = set()
            for c in per_t:
                seen |= ngc.features(kind, q0, q1, c)
                rec = records(kind, c)
                counts.add(len(rec))
                pos |= {o % K_BACK for o, r in enumerate(rec) if r == "z"}
            differ = differ or len(counts) > 1
    return seen, pos, differ, margin


# ---- the Z-heavy table case (n = 14) ----------------------------------------------------------------------------------------
W1 = np.array([0.02, 0.03, 0.25])
W2 = np.full(15, 0.004)
W2[[3 - 1, 12 - 1, 15 - 1]] = 0.08
TABLE_P = (0.5, 0.5)            # p1 / p2 of set_noise that the tables must replace
TABLE_SEED = 4321


# ---- the L-BFGS case (n = 14): small p, float32-exact start angles ------------------------------------------------------------
LBFGS_P = (0.05, 0.08)
_LB = {}


def lbfgs_case():
    if "c" not in _LB:
        n = 14
        rng = np.random.default_rng(1466)
        psi0, ham = random_state(n, rng), random_hamiltonian(n, 10, rng)
        circuits = []
        for _ in range(2):
            kind, q0, q1, pidx, th = random_gates(n, 10, rng, p_cnot=0.35)
            circuits.append((with_noise_gates(kind, q0, q1, pidx), th.astype(np.float32).astype(np.float64)))
        _LB["c"] = {"n": n, "psi0": psi0, "ham": ham, "scale": ngc.scale(ham), "circuits": circuits}
    return _LB["c"]
