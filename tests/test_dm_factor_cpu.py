"""CPU: the factorised oracle of the exact channel mode (tests/dm_factor_oracle.py) against the full one
(vo.run_circuit_dm / vo.energy_dm, helpers.shift_grad) at the sizes the full one still serves, and the properties of its
partitions and circuits that tests/test_dm_large_gpu.py relies on at 9-13 qubits.

Bounds: |dE| <= 1e-13 and |dg| <= 1e-13 max(1, sum |c|) - both sides are sums of O(2^n) products of numbers below 1 in
double precision; observed 1e-17 .. 1e-16."""
import functools
import itertools

import numpy as np
import pytest

import dm_factor_oracle as fo
import vqe_oracle as vo
from helpers import random_hamiltonian, shift_grad

E_BOUND = 1e-13

# (n, partition): two and three factors, no set contiguous
CASES = [(4, [[0, 2], [1, 3]]), (6, [[0, 3, 5], [1, 2, 4]]), (6, [[0, 5], [1, 3], [2, 4]]), (7, [[0, 4], [1, 3, 6], [2, 5]]),
         (7, [[0, 2, 3, 6], [1, 4, 5]]), (8, [[0, 3, 7], [1, 2, 4, 5, 6]]), (8, [[0, 6], [1, 4, 7], [2, 3, 5]])]
NOISE = [(0.2, 0.3), (0.01, 0.05)]


@functools.lru_cache(maxsize=None)
def _case(i):
    n, parts = CASES[i]
    rng = np.random.default_rng(9900 + i)
    psi0, states = fo.product_state(n, parts, rng)
    ham = random_hamiltonian(n, 30, rng, real=False)
    pairs = [tuple(int(q) for q in rng.permutation(s)[:2]) for s in parts]
    # (the full oracle takes 30 ms per gate at 8 qubits, and the shift rule two evaluations per rotation)
    circuit = fo.factor_gates(n, parts, {7: 10, 8: 8}.get(n, 20), rng, p_cnot=0.4, required_pairs=pairs)
    return n, parts, psi0, states, ham, circuit


def test_product_state_is_the_tensor_product():
    n, parts = 5, [[0, 3], [1, 2, 4]]
    psi, (a, b) = fo.product_state(n, parts, np.random.default_rng(1))
    assert abs(np.vdot(psi, psi) - 1.0) < 1e-14
    for i in range(1 << n):
        ia = ((i >> 0) & 1) | (((i >> 3) & 1) << 1)
        ib = ((i >> 1) & 1) | (((i >> 2) & 1) << 1) | (((i >> 4) & 1) << 2)
        assert abs(psi[i] - a[ia] * b[ib]) < 1e-16
    # the factor states of a coarser partition: the same full vector
    fine = [[0], [3], [1, 4], [2]]
    psi, states = fo.product_state(n, fine, np.random.default_rng(2))
    again = np.ones(1 << n, np.complex128)
    for s, phi in zip(parts, fo.coarsen(fine, states, parts)):
        again = again * phi[fo._local_index(n, s)]
    assert np.abs(again - psi).max() < 1e-16


@pytest.mark.parametrize("i", range(len(CASES)))
@pytest.mark.parametrize("p1,p2", NOISE)
def test_factorised_energy_matches_the_full_oracle(i, p1, p2):
    n, parts, psi0, states, ham, c = _case(i)
    assert any(bin(int(x) & int(z)).count("1") % 2 for x, z in zip(ham[0], ham[1]))       # odd numbers of Y
    assert any(list(s) != list(range(s[0], s[0] + len(s))) for s in parts)                # sets that are not contiguous
    assert not fo.crosses(parts, c) and np.any(c[0] == 5) and np.any(c[0] == 4)
    rng = np.random.default_rng(50 + i)
    worst = 0.0
    for theta in (c[4], c[4] + rng.normal(size=c[4].size)):
        full = vo.energy_dm(vo.run_circuit_dm(psi0, *c[:4], theta, p1, p2), *ham)
        worst = max(worst, abs(fo.energy(n, parts, states, c[:4], theta, ham, p1, p2) - full))
    keep = c[0] < 4
    clean = vo.energy_pauli(vo.run_circuit(psi0, c[0][keep], c[1][keep], c[2][keep], c[3][keep], c[4]), *ham)
    d_clean = abs(fo.energy(n, parts, states, c[:4], c[4], ham, p1, p2, noiseless=True) - clean)
    print(f"n={n} {len(parts)} factors p=({p1}, {p2}): |dE|={worst:.1e} noiseless |dE|={d_clean:.1e} noise moves E by {abs(full - clean):.2e}")
    assert worst <= E_BOUND and d_clean <= E_BOUND
    assert abs(full - clean) > 1e-6                            # the channels matter: the comparison is not vacuous


@pytest.mark.parametrize("i", [0, 1, 3, 5])
@pytest.mark.parametrize("p1,p2", NOISE)
def test_factorised_shift_gradient_matches_the_full_oracle(i, p1, p2):
    n, parts, psi0, states, ham, c = _case(i)
    # one parameter shared by two gates, one unused
    pidx = c[3].copy()
    last = int(pidx.max())
    pidx[pidx == last] = 0
    assert np.count_nonzero(pidx == 0) == 2
    dm = lambda psi, k, a, b, p, th, h: vo.energy_dm(vo.run_circuit_dm(psi, k, a, b, p, th, p1, p2), *h)
    full = shift_grad(psi0, c[0], c[1], c[2], pidx, c[4], ham, energy=dm)
    e, g = fo.shift_grad(n, parts, states, (c[0], c[1], c[2], pidx), c[4], ham, p1, p2)
    scale = max(1.0, float(np.abs(ham[2]).sum()))
    print(f"n={n} {len(parts)} factors p=({p1}, {p2}): |dg|={np.abs(g - full).max():.1e} of {E_BOUND * scale:.1e}, max|g|={np.abs(full).max():.2e}")
    assert abs(e - dm(psi0, c[0], c[1], c[2], pidx, c[4], ham)) <= E_BOUND
    assert np.abs(g - full).max() <= E_BOUND * scale
    assert g[last] == 0.0 and np.abs(full).max() > 1e6 * E_BOUND * scale          # far above the bound: not a row of zeros


@pytest.mark.parametrize("n", [9, 10, 11, 12, 13])
def test_covering_partitions_reach_every_pair(n):
    for seed in range(5):
        three = fo.covering_partitions(n, np.random.default_rng(seed))
        assert len(three) == 3
        for parts in three:
            assert sorted(q for s in parts for q in s) == list(range(n)) and len(parts) == 2
            assert max(len(s) for s in parts) <= 7
        for a, b in itertools.combinations(range(n), 2):
            assert any(fo.set_of(parts, a) == fo.set_of(parts, b) for parts in three), (a, b, three)
        fine = fo.refinement(three)
        assert len(fine) == 4 and sorted(len(s) for s in fine) == sorted(n // 4 + (i < n % 4) for i in range(4))
        assert all(any(set(c) <= set(s) for s in parts) for c in fine for parts in three)
    assert any(list(s) != list(range(s[0], s[0] + len(s))) for parts in three for s in parts)


def test_factor_gates_never_cross_a_set():
    rng = np.random.default_rng(7)
    for n in (6, 9, 13):
        for parts in fo.covering_partitions(n, rng):
            pairs = [(a, b) for s in parts for a, b in itertools.permutations(s, 2)][::3]
            c = fo.factor_gates(n, parts, 40, rng, p_cnot=0.6, required_pairs=pairs)
            kind, q0, q1, pidx, theta = c
            assert not fo.crosses(parts, c)
            assert np.count_nonzero(kind == 0) >= len(pairs) and kind.size == 2 * (40 + 2 * len(pairs))
            # the required CNOTs are there, in their order; a channel sits behind every gate; every rotation has an angle
            cnots = [(int(a), int(b)) for k, a, b in zip(kind, q0, q1) if k == 0]
            it = iter(cnots)
            assert all(p in it for p in pairs)
            assert np.all(kind[1::2] == np.where(kind[0::2] == 0, 5, 4)) and np.all(q0[1::2] == q0[0::2])
            assert sorted(pidx[pidx >= 0].tolist()) == list(range(theta.size))
    # a crossing gate is seen
    parts = [[0, 2], [1, 3]]
    bad = (np.array([0], np.int32), np.array([0], np.int32), np.array([1], np.int32), np.array([-1], np.int32))
    assert fo.crosses(parts, bad) == [0]
    with pytest.raises(AssertionError):
        fo.restrict_circuit(parts[0], bad)
