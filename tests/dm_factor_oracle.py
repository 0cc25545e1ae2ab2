"""A factorised oracle of the exact channel mode, exact and cheap at any qubit count (tests/test_dm_factor_cpu.py holds
it against the full oracle; tests/test_dm_large_gpu.py uses it at 9-13 qubits, where vo.run_circuit_dm takes minutes).

Split the qubits into disjoint sets S_1 .. S_m (not contiguous), start from a product state over the sets and keep every
gate and every channel inside one set.  Then rho = rho_1 (x) .. (x) rho_m exactly, whatever the interleaving of the
gates, tr(rho P) = prod_f tr(rho_f P_f) for a Pauli string P with restrictions P_f (each with its own i^#Y), and
    E = sum_k c_k prod_f e_kf,     e_kf = vo.energy_dm(rho_f, [x_kf], [z_kf], [1.0]),
with rho_f from vo.run_circuit_dm on |S_f| <= 7 qubits.  The Hamiltonian is unrestricted and the library knows nothing
of the partition: its windows, block fusion and sweeps act on the full 4^n matrix.

Conventions: a partition is a list of sorted qubit lists; local bit j of factor f is qubit parts[f][j] (little-endian,
as everywhere in the oracle); a circuit is (kind, q0, q1, pidx) in the project's layout with global qubits and global
parameter indices.  numpy + vqe_oracle only."""
import numpy as np

import vqe_oracle as vo
from helpers import random_state, with_noise_gates


def _local_index(n, part):
    """for every basis index of n qubits, the index of its bits on `part`"""
    idx = np.arange(1 << n, dtype=np.int64)
    loc = np.zeros_like(idx)
    for j, q in enumerate(part):
        loc |= ((idx >> q) & 1) << j
    return loc


def _check_partition(n, parts):
    flat = sorted(q for s in parts for q in s)
    assert flat == list(range(n)), (n, parts)
    assert all(list(s) == sorted(s) for s in parts), parts


def product_state(n, parts, rng):
    """-> (the full 2^n vector for set_init_state, the factor states): a random state on every set"""
    _check_partition(n, parts)
    states = [random_state(len(s), rng) for s in parts]
    psi = np.ones(1 << n, np.complex128)
    for s, phi in zip(parts, states):
        psi = psi * phi[_local_index(n, s)]
    return psi, states


def refinement(partitions):
    """The coarsest partition that refines every one of `partitions`: qubits that share a set in all of them."""
    n = sum(len(s) for s in partitions[0])
    key = lambda q: tuple(next(i for i, s in enumerate(p) if q in s) for p in partitions)
    classes = {}
    for q in range(n):
        classes.setdefault(key(q), []).append(q)
    return sorted(classes.values())


def coarsen(fine, fine_states, parts):
    """Factor states of `parts` from those of the finer partition `fine` (every set of `fine` inside one of `parts`)."""
    out = []
    for s in parts:
        inside = [(c, phi) for c, phi in zip(fine, fine_states) if set(c) <= set(s)]
        assert sorted(q for c, _ in inside for q in c) == list(s), (fine, parts)
        psi = np.ones(1 << len(s), np.complex128)
        for c, phi in inside:
            psi = psi * phi[_local_index(len(s), [s.index(q) for q in c])]
        out.append(psi)
    return out


def covering_partitions(n, rng):
    """Three partitions of range(n) into two sets each, such that every pair of qubits shares a set in at least one:
    four classes C0 .. C3 of a seeded shuffle (sizes as equal as possible, the larger ones first: 3,3,3,3 at n = 12,
    4,3,3,3 at n = 13) and {C0 u C1 | C2 u C3}, {C0 u C2 | C1 u C3}, {C0 u C3 | C1 u C2}."""
    assert n >= 4
    order = [int(q) for q in rng.permutation(n)]
    size = [n // 4 + (1 if i < n % 4 else 0) for i in range(4)]
    cut = np.concatenate([[0], np.cumsum(size)])
    c = [order[cut[i]:cut[i + 1]] for i in range(4)]
    return [[sorted(c[0] + c[i]), sorted(sum((c[j] for j in (1, 2, 3) if j != i), []))] for i in (1, 2, 3)]


def set_of(parts, q):
    return next(i for i, s in enumerate(parts) if q in s)


def factor_gates(n, parts, G, rng, p_cnot=0.5, required_pairs=()):
    """A noisy circuit whose gates never cross a set of `parts`: -> (kind, q0, q1, pidx, theta) with DEPOL2 behind every
    CNOT and DEPOL1 behind every rotation (helpers.with_noise_gates), every rotation a parameter of its own.
    ``required_pairs``: ordered (control, target) pairs, each inside one set; their CNOTs come in the given order, each
    followed by a rotation on its target (consecutive CNOTs on one pair of qubits thus stay in one two-qubit window).
    The G random gates (a set drawn by its size, then a CNOT with probability p_cnot or a rotation) land at random
    places between them."""
    _check_partition(n, parts)
    gates = []                                   # (kind, q0, q1)
    for c, t in required_pairs:
        assert c != t and set_of(parts, c) == set_of(parts, t), (c, t, parts)
        gates.append([(0, int(c), int(t)), (1 + int(rng.integers(3)), int(t), -1)])
    weights = np.array([len(s) for s in parts], float) / n
    for _ in range(G):
        s = parts[int(rng.choice(len(parts), p=weights))]
        if rng.random() < p_cnot and len(s) > 1:
            c, t = (int(q) for q in rng.choice(s, 2, replace=False))
            g = (0, c, t)
        else:
            g = (1 + int(rng.integers(3)), int(rng.choice(s)), -1)
        gates.insert(int(rng.integers(len(gates) + 1)), [g])
    kind, q0, q1, pidx = [], [], [], []
    for k, a, b in (g for group in gates for g in group):
        kind.append(k), q0.append(a), q1.append(b)
        pidx.append(-1 if k == 0 else sum(1 for p in pidx if p >= 0))
    theta = rng.uniform(-np.pi, np.pi, sum(1 for p in pidx if p >= 0))
    return with_noise_gates(kind, q0, q1, pidx) + (theta,)


def crosses(parts, circuit):
    """the gates of `circuit` whose qubits do not lie in one set"""
    kind, q0, q1 = circuit[:3]
    return [g for g in range(len(kind)) if q1[g] >= 0 and set_of(parts, int(q0[g])) != set_of(parts, int(q1[g]))]


def restrict_circuit(part, circuit):
    """The gates of `circuit` on the qubits of `part`, renumbered to its local bits (parameter indices stay global)."""
    kind, q0, q1, pidx = (np.asarray(v) for v in circuit[:4])
    local = {q: j for j, q in enumerate(part)}
    keep = [g for g in range(kind.size) if int(q0[g]) in local]
    assert all(q1[g] < 0 or int(q1[g]) in local for g in keep), "a gate crosses the partition"
    return (np.array([kind[g] for g in keep], np.int32), np.array([local[int(q0[g])] for g in keep], np.int32),
            np.array([local[int(q1[g])] if q1[g] >= 0 else -1 for g in keep], np.int32),
            np.array([pidx[g] for g in keep], np.int32))


def restrict_term(part, x, z):
    x, z = int(x), int(z)
    return (sum(((x >> q) & 1) << j for j, q in enumerate(part)), sum(((z >> q) & 1) << j for j, q in enumerate(part)))


def factor_expectations(part, state, circuit, theta, ham, p1, p2, noiseless=False):
    """e_kf for every term k of `ham` on one factor: tr(rho_f P_kf), or <psi_f| P_kf |psi_f> of the circuit without its
    channels when ``noiseless``."""
    k, a, b, p = restrict_circuit(part, circuit)
    terms = [restrict_term(part, x, z) for x, z in zip(ham[0], ham[1])]
    cache = {}
    if noiseless:
        psi = vo.run_circuit(state, k, a, b, p, theta)           # channels are the identity without draws
        one = lambda x, z: vo.energy_pauli(psi, np.array([x], np.uint64), np.array([z], np.uint64), np.array([1.0]))
    else:
        rho = vo.run_circuit_dm(state, k, a, b, p, theta, p1, p2)
        one = lambda x, z: vo.energy_dm(rho, [x], [z], [1.0])
    for t in terms:
        if t not in cache:
            cache[t] = one(*t)
    return np.array([cache[t] for t in terms])


def energy(n, parts, factor_states, circuit, theta, ham, p1, p2, noiseless=False):
    """E = sum_k c_k prod_f e_kf of the circuit (kind, q0, q1, pidx) at theta; ``noiseless``: the same circuit without its
    channels, from the factor state vectors."""
    _check_partition(n, parts)
    theta = np.asarray(theta, np.float64)
    e = np.ones(len(ham[2]))
    for s, phi in zip(parts, factor_states):
        e = e * factor_expectations(s, phi, circuit, theta, ham, p1, p2, noiseless)
    return float(np.dot(np.asarray(ham[2], np.float64), e))


def shift_grad(n, parts, factor_states, circuit, theta, ham, p1, p2):
    """The exact parameter shift of helpers.shift_grad over the factorised energy: gate by gate, +-pi/2, each gate its
    own copy of the angle, summed into the gate's parameter.  A shifted gate changes the factor it lives in alone, so
    only that factor's e_kf are evaluated again.  -> (E, dE/dtheta)"""
    _check_partition(n, parts)
    kind, q0, q1, pidx = (np.asarray(v) for v in circuit[:4])
    theta = np.asarray(theta, np.float64)
    c = np.asarray(ham[2], np.float64)
    rot = [g for g in range(kind.size) if kind[g] in (1, 2, 3)]
    own = np.full(kind.size, -1, np.int32)
    for i, g in enumerate(rot):
        own[g] = i
    base = np.array([theta[pidx[g]] for g in rot])
    private = (kind, q0, q1, own)
    e = [factor_expectations(s, phi, private, base, ham, p1, p2) for s, phi in zip(parts, factor_states)]
    grad = np.zeros(theta.size)
    for i, g in enumerate(rot):
        f = set_of(parts, int(q0[g]))
        rest = np.prod([e[j] for j in range(len(parts)) if j != f], axis=0) if len(parts) > 1 else np.ones(c.size)
        d = 0.0
        for sign in (1.0, -1.0):
            t = base.copy()
            t[i] += sign * np.pi / 2
            d += sign * float(np.dot(c, rest * factor_expectations(parts[f], factor_states[f], private, t, ham, p1, p2)))
        grad[pidx[g]] += 0.5 * d
    return float(np.dot(c, np.prod(e, axis=0))), grad
