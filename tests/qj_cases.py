"""Cases shared by tests/test_kraus_traj_cpu.py and tests/test_kraus_traj_gpu.py (a helper, not a test): the channel
combinations, the circuits and the seeds.  The seeds were chosen on the CPU, on the oracle (tests/qj_oracle.py) alone, so
that the two preconditions of the per-trajectory parity test hold with no trajectory left out - every draw at least
1e-9 from a boundary of its cumulative distribution, every Kraus index of every set chosen at least once - and so that
the distribution case's mean lies within 3 sem of the exact channel; the CPU tests assert that they do."""
import numpy as np

import qj_oracle as qo
from su4_helpers import random_gates_su4

S = np.sqrt


def amplitude_damping(g):
    return np.array([[[1, 0], [0, S(1 - g)]], [[0, S(g)], [0, 0]]], np.complex128)


def dephasing(p):
    return np.stack([S(1 - p) * qo.PAULI[0], S(p) * qo.PAULI[3]])


def tensor(Ka, Kb):
    """Ka on q0 (the low index bit), Kb on q1"""
    return np.stack([np.kron(b, a) for a in Ka for b in Kb])


def combo(name):
    if name == "damping+product":
        return amplitude_damping(0.3), tensor(amplitude_damping(0.25), dephasing(0.2))
    if name == "dephasing+cnot":      # the non-product, non-symmetric set {sqrt 0.7 1, sqrt 0.3 CNOT(q0 -> q1)}
        return dephasing(0.2), np.stack([S(0.7) * np.eye(4, dtype=np.complex128), S(0.3) * qo.CX])
    raise KeyError(name)


COMBOS = ("damping+product", "dephasing+cnot")
PARITY_N = (2, 5, 7, 9, 10, 12, 13)
PARITY_T, PARITY_EVALS, PARITY_BATCH, PARITY_GATES = 8, 3, 3, 24
PARITY_SEED = 20251
MARGIN = 1e-9

# the n = 3 circuit of test_noise_statistics_match_depolarizing_channels (tests/test_hip_parity.py)
DIST_SEED, DIST_T, DIST_EVALS = 424242, 4096, 6


def noisy_su4(n, G, rng):
    """G gates of all nine kinds (every kind present, CNOTs among them so that the frame's map is not the identity) with
    a noise gate behind every gate: DEPOL2 on the gate's (q0, q1) behind a two-qubit gate, DEPOL1 behind a rotation."""
    while True:
        k, a, b, p, th = random_gates_su4(n, G, rng)
        if n < 2 or set(int(v) for v in k) >= {0, 1, 2, 3, 6, 7, 8}:
            break
    kind, q0, q1, pidx = [], [], [], []
    for kk, aa, bb, pp in zip(k, a, b, p):
        two = int(kk) in (0, 6, 7, 8)
        kind += [int(kk), 5 if two else 4]
        q0 += [int(aa), int(aa)]
        q1 += [int(bb), int(bb) if two else -1]
        pidx += [int(pp), -1]
    return tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)) + (th,)


def parity_case(n):
    """psi0, ham, the batch of circuits"""
    from helpers import random_hamiltonian, random_state
    rng = np.random.default_rng(7700 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 14, rng, real=False)
    return psi0, ham, [noisy_su4(n, PARITY_GATES, rng) for _ in range(PARITY_BATCH)]


def dist_case():
    from helpers import random_hamiltonian, random_state
    n = 3
    rng = np.random.default_rng(5)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 12, rng)
    c = (np.array([1, 4, 0, 5, 2, 4], np.int32), np.array([0, 0, 0, 0, 2, 2], np.int32), np.array([-1, -1, 1, 1, -1, -1], np.int32),
         np.array([0, -1, -1, -1, 1, -1], np.int32), np.array([0.7, -1.3]))
    return psi0, ham, c


def oracle_runs(psi0, ham, circuits, K1, K2, seed, evals, T, thetas=None, first_eval=0):
    """[evaluation][circuit] -> qj_oracle.run"""
    return [[qo.run(psi0, c[0], c[1], c[2], c[3], c[4] if thetas is None else thetas[b], K1, K2, ham, seed, b, first_eval + e, T)
             for b, c in enumerate(circuits)] for e in range(evals)]


def assert_preconditions(runs, K1, K2):
    """on the oracle alone: every draw at least MARGIN from a boundary, every Kraus index of both sets chosen"""
    seen = {1: set(), 2: set()}
    for ev in runs:
        for r in ev:
            assert r["margin"] >= MARGIN
            for kind in (1, 2):
                seen[kind] |= set(r["ks"][:, r["slot_kind"] == kind].ravel().tolist())
    assert seen[1] == set(range(len(K1))) and seen[2] == set(range(len(K2))), seen
