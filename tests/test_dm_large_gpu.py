"""GPU: the exact channel mode at 9-13 qubits, every path against an exact value: the serial path (k_dm_block,
k_dm_energy, k_dm_sum: the path bench.py times at 12 qubits), the batched path (vqe_dm_batch.h), the adjoint gradient
(vqe_dm_grad.h) and the device L-BFGS on it, all WITH noise.

Reference: the factorised oracle of tests/dm_factor_oracle.py (held against the full oracle by
tests/test_dm_factor_cpu.py): product initial state, every gate and channel inside one set of a partition of the qubits,
E = sum_k c_k prod_f tr(rho_f P_kf) with factors of at most 7 qubits from vo.run_circuit_dm.  The library is not told of
the partition.  One partition reaches only the qubit pairs inside its sets; the three of fo.covering_partitions reach
every pair, so every two-qubit window of rho is swept with noise somewhere.

What the sizes reach that 2-8 qubits (and 10 with one workgroup trip) do not: k_dm_block's grid-stride trip (4^n / 1024
workgroups wanted, 8 per CU launched: from 11 qubits on), window bits above bit 15 and n_groups >= 2^18 (from 11), the
gradient's tiles per partial above its floor of 4 (16, 64, 256, 1024 at 10 .. 13) and its 256 partials (from 9).

Tolerances: the project's own - energies 1e-10 (tests/test_dm_gpu.py), gradients and their E 1e-10 max(1, sum |c_k|)
(tests/test_dm_grad_gpu.py)."""
import functools
import itertools

import numpy as np
import pytest

import dm_factor_oracle as fo
import vqe_oracle as vo
from helpers import random_hamiltonian

pytestmark = pytest.mark.gpu
E_TOL = 1e-10
NOISE = {"reference": (0.01, 0.05), "strong": (0.1, 0.2)}      # the noisy environments' strengths, and ten / four times them
GIB = 1 << 30


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _engine(tq, n, psi0, ham, p1, p2, batched=None, grad=False):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(p1, p2, 11)
    eng.set_noise_mode(1)
    if batched is not None:
        eng.set_dm_batched(batched)
    if grad:
        eng.set_dm_grad()
    return eng


def _circ(tq, c):
    return tq.Circuit(c[0], c[1], c[2], c[3], c[4].size)


def _scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


def _n_blocks(n, c, p1, p2):
    """the block count of vqe_dm_plan (host only)"""
    import ctypes as C
    from tensorrl_qas_amd import _lib
    nb = C.c_int32()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib.c_i32p)
    th = np.ascontiguousarray(c[4] if c[4].size else np.zeros(1))
    assert _lib.load().vqe_dm_plan(n, len(c[0]), i32(c[0]), i32(c[1]), i32(c[2]), i32(c[3]), th.ctypes.data_as(_lib.c_f64p),
                                   p1, p2, 0, C.byref(nb), None, None) == 0
    return nb.value


@functools.lru_cache(maxsize=None)
def _problem(n):
    """The three covering partitions of n qubits, a product state over their common refinement (so it is a product state
    of every one of them, and one handle serves all three), its factor states per partition, and a Hamiltonian with
    complex sign-sum coefficients.  Made once, shared, never modified."""
    rng = np.random.default_rng(9700 + n)
    three = fo.covering_partitions(n, rng)
    fine = fo.refinement(three)
    psi0, fine_states = fo.product_state(n, fine, rng)
    states = [fo.coarsen(fine, fine_states, parts) for parts in three]
    ham = random_hamiltonian(n, 30, rng, real=False)
    assert any(bin(int(x) & int(z)).count("1") % 2 for x, z in zip(ham[0], ham[1]))      # complex coefficients
    return three, states, psi0, ham


@functools.lru_cache(maxsize=None)
def _covering_case(n):
    """One circuit per covering partition: CNOTs on EVERY pair of qubits inside its sets, control and target in both
    orders, a rotation behind every CNOT (so on every qubit), and 0 / 1 / 2 more gates so that the lengths differ; the
    nominal angles and two perturbed vectors.  A pair's two CNOTs and their rotations share one window: one block per
    pair (36 at 13 qubits, where a sweep moves 2 GiB)."""
    three, states, psi0, ham = _problem(n)
    rng = np.random.default_rng(9720 + n)
    circuits, thetas = [], []
    for i, parts in enumerate(three):
        pairs = [tuple(int(q) for q in rng.permutation(p)) for s in parts for p in itertools.combinations(s, 2)]
        pairs = [pairs[j] for j in rng.permutation(len(pairs))]
        c = fo.factor_gates(n, parts, i, rng, required_pairs=[o for a, b in pairs for o in ((a, b), (b, a))])
        circuits.append(c)
        thetas.append(np.stack([c[4], c[4] + rng.normal(size=c[4].size), c[4] + rng.normal(size=c[4].size)]))
    return circuits, thetas


@functools.lru_cache(maxsize=None)
def _covering_oracle(n, noise):
    """-> (channel energies [partition][theta], noiseless energies at the nominal angles [partition])"""
    three, states, psi0, ham = _problem(n)
    circuits, thetas = _covering_case(n)
    p1, p2 = NOISE[noise]
    ref = np.array([[fo.energy(n, parts, st, c[:4], t, ham, p1, p2) for t in ths]
                    for parts, st, c, ths in zip(three, states, circuits, thetas)])
    clean = np.array([fo.energy(n, parts, st, c[:4], c[4], ham, p1, p2, noiseless=True) for parts, st, c in zip(three, states, circuits)])
    return ref, clean


@functools.lru_cache(maxsize=None)
def _serial(tq, n, noise):
    """The serial path's energies of the covering circuits [partition][theta] and its block counts: run once, shared by
    the serial and the batched test."""
    three, states, psi0, ham = _problem(n)
    circuits, thetas = _covering_case(n)
    eng = _engine(tq, n, psi0, ham, *NOISE[noise])
    got, blocks = [], []
    for c, ths in zip(circuits, thetas):
        eng.set_circuit(_circ(tq, c))
        got.append(eng.energy_batch(ths))
        blocks.append(eng.noise_mode_info()["blocks_last_evaluation"])
    assert eng.dm_batch_info() == {"resident": 0, "chunks": 0, "evaluations": 0, "levels": 0}      # the serial path
    return np.array(got), blocks, eng.device_info()["cu_count"]


def _ordered_cnots(c):
    return {(int(a), int(b)) for k, a, b in zip(c[0], c[1], c[2]) if k == 0}


# ---- a. the serial path ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", list(NOISE))
@pytest.mark.parametrize("n", [9, 10, 11, 12, 13])
def test_serial_path_on_every_window(tq, n, noise):
    """At the reference strengths the energies of these deep circuits are 1e-5 .. 1e-2: four to eight of their digits are
    checked.  At the strong pair every Pauli term has decayed to 1e-5 .. 1e-10: what that case holds is that NOTHING of
    rho escapes a sweep - an entry that a block misses keeps its undamped size (1e-2, the noiseless energies)."""
    three, states, psi0, ham = _problem(n)
    circuits, thetas = _covering_case(n)
    p1, p2 = NOISE[noise]
    # every ordered pair of qubits is a CNOT of one of the three circuits, (0, 1), (n - 2, n - 1) and (0, n - 1) among them;
    # every qubit is rotated in every circuit; no gate leaves its set
    union = set().union(*(_ordered_cnots(c) for c in circuits))
    assert union == set(itertools.permutations(range(n), 2))
    for parts, c in zip(three, circuits):
        assert not fo.crosses(parts, c) and set(c[1][(c[0] >= 1) & (c[0] <= 3)].tolist()) == set(range(n))
    assert len({len(c[0]) for c in circuits}) == 3
    plan = [_n_blocks(n, c, p1, p2) for c in circuits]
    assert n < 13 or max(plan) <= 40, plan
    got, blocks, cus = _serial(tq, n, noise)
    assert blocks == plan, (blocks, plan)
    if n >= 11:
        # the reason for these sizes: k_dm_block wants 4^n / 1024 workgroups and gets 8 per CU, so a wave makes more than
        # one trip of its loop over the tiles.  On a device where this fails the test has lost its point at this n.
        assert 4 ** n // 1024 > 8 * cus, (n, cus)
    ref, clean = _covering_oracle(n, noise)
    err = np.abs(got - ref)
    print(f"serial n={n} p=({p1}, {p2}): worst |dE|={err.max():.2e} ({err.max() / E_TOL:.1e} of the bound), blocks {blocks}, "
          f"E {ref[:, 0]}, noiseless {clean}")
    assert err.max() < E_TOL, (got, ref)
    assert np.abs(clean - ref[:, 0]).min() > 1e-6                        # the channels move every energy: not vacuous
    assert noise != "reference" or np.abs(ref[:, 0]).min() > 1e4 * E_TOL


# ---- b. the batched path -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", list(NOISE))
@pytest.mark.parametrize("n", [9, 11, 12, 13])
def test_batched_path_on_every_window(tq, n, noise):
    """The three covering circuits (unequal lengths) and one circuit with zero gates in one batch: what fits, all four resident, then
    one at a time - the same bits (vqe_dm_batch.h: a circuit's bits do not depend on the batch around it)."""
    three, states, psi0, ham = _problem(n)
    circuits, thetas = _covering_case(n)
    p1, p2 = NOISE[noise]
    empty = tuple(np.zeros(0, np.int32) for _ in range(4)) + (np.zeros(0),)
    batch = circuits + [empty]
    assert len({len(c[0]) for c in batch}) == 4
    ref, clean = _covering_oracle(n, noise)
    ref = np.append(ref[:, 0], vo.energy_pauli(psi0, *ham))
    eng = _engine(tq, n, psi0, ham, p1, p2, batched=-1)
    got = {}
    for R in (-1, 4, 1):
        eng.set_dm_batched(R)
        eng.batch_load([_circ(tq, c) for c in batch], [c[4] for c in batch])
        eng.batch_run_energy()
        got[R] = eng.batch_fetch(want_x=False)[1].copy()
        info = eng.dm_batch_info()
        # (-1 holds what fits a quarter of the memory that is free: all four, unless the card is nearly full - hence R = 4)
        assert (1 <= info["resident"] <= 4 if R < 0 else info["resident"] == R) and info["chunks"] == -(-4 // info["resident"]), info
        assert info["evaluations"] == 1 and info["levels"] == max(_n_blocks(n, c, p1, p2) for c in circuits), info
    err = np.abs(got[-1] - ref)
    serial = _serial(tq, n, noise)[0][:, 0]
    print(f"batched n={n} p=({p1}, {p2}): worst |dE|={err.max():.2e} ({err.max() / E_TOL:.1e} of the bound), "
          f"against the serial path {np.abs(got[-1][:3] - serial).max():.2e}")
    assert err.max() < E_TOL, (got[-1], ref)
    assert np.array_equal(got[-1], got[1]) and np.array_equal(got[4], got[1]), (got[-1], got[4], got[1])
    assert np.abs(got[-1][:3] - serial).max() <= 1e-12                    # (bits are not promised across the two paths)
    assert np.abs(clean - ref[:3]).min() > 1e-6


# ---- c. the adjoint gradient ---------------------------------------------------------------------------------------------

# n -> the random gates of the two circuits (beside the CNOTs and rotations on two required pairs each).  13 qubits:
# a density matrix is 1 GiB and a resident circuit keeps levels + 2 of them, so at most 6 blocks per circuit.
GRAD_GATES = {9: (14, 9), 11: (12, 7), 12: (10, 6), 13: (3, 1)}


@functools.lru_cache(maxsize=None)
def _grad_case(n):
    """Two circuits from different partitions with unequal parameter counts; in each, the last parameter's gate takes
    parameter 0 instead: one parameter shared by two gates, one unused."""
    three, states, psi0, ham = _problem(n)
    rng = np.random.default_rng(9740 + n)
    out = []
    for which, G in zip((0, 2), GRAD_GATES[n]):
        parts = three[which]
        pairs = [tuple(int(q) for q in rng.permutation(s)[:2]) for s in parts]
        kind, q0, q1, pidx, th = fo.factor_gates(n, parts, G, rng, p_cnot=0.3, required_pairs=pairs)
        last = int(pidx.max())
        assert last >= 2
        pidx = np.where(pidx == last, 0, pidx).astype(np.int32)
        out.append((which, (kind, q0, q1, pidx, th)))
    assert out[0][1][4].size != out[1][1][4].size
    return out


@functools.lru_cache(maxsize=None)
def _grad_oracle(n, noise):
    three, states, psi0, ham = _problem(n)
    p1, p2 = NOISE[noise]
    ref = [fo.shift_grad(n, three[w], states[w], c[:4], c[4], ham, p1, p2) for w, c in _grad_case(n)]
    clean = [fo.energy(n, three[w], states[w], c[:4], c[4], ham, p1, p2, noiseless=True) for w, c in _grad_case(n)]
    return ref, clean


@pytest.mark.parametrize("noise", list(NOISE))
@pytest.mark.parametrize("n", [9, 11, 12, 13])
def test_gradient_against_the_factorised_shift_rule(tq, n, noise):
    three, states, psi0, ham = _problem(n)
    p1, p2 = NOISE[noise]
    circuits = [c for _, c in _grad_case(n)]
    for (w, c) in _grad_case(n):
        assert not fo.crosses(three[w], c)
        assert np.count_nonzero(c[3] == 0) == 2 and not np.any(c[3] == c[4].size - 1)      # shared, unused
    # memory is a condition: levels + 2 density matrices per resident circuit, both circuits resident, 16 GiB at most;
    # the budget is given explicitly, so it is not a quarter of what happens to be free on the card
    levels = max(_n_blocks(n, c, p1, p2) for c in circuits)
    resident = 2
    assert (levels + 2) * 16 * 4 ** n * resident <= 16 * GIB, (n, levels)
    eng = _engine(tq, n, psi0, ham, p1, p2, batched=resident * (levels + 2), grad=True)
    eng.batch_load([_circ(tq, c) for c in circuits], [c[4] for c in circuits])
    eng.batch_run_energy_grad()
    f = eng.batch_fetch(want_x=False)[1].copy()
    g = eng.batch_fetch_grad()
    assert eng.dm_batch_info() == {"resident": resident, "chunks": 1, "evaluations": 1, "levels": levels}, eng.dm_batch_info()
    eng.batch_run_energy()
    assert np.array_equal(eng.batch_fetch(want_x=False)[1], f)            # E is the energy run's, bit for bit
    ref, clean = _grad_oracle(n, noise)
    scale = _scale(ham)
    off = 0
    for b, (c, (e_ref, g_ref)) in enumerate(zip(circuits, ref)):
        P = c[4].size
        gb = g[off:off + P]
        off += P
        de, dg = abs(f[b] - e_ref), np.abs(gb - g_ref).max()
        print(f"gradient n={n} p=({p1}, {p2}) circuit {b} (P={P}, {_n_blocks(n, c, p1, p2)} blocks): |dE|={de:.2e} "
              f"({de / (E_TOL * scale):.1e} of the bound) |dg|={dg:.2e} ({dg / (E_TOL * scale):.1e}) max|g|={np.abs(g_ref).max():.2e}")
        assert de <= E_TOL * scale, (b, f[b], e_ref)
        assert dg <= E_TOL * scale, (b, gb, g_ref)
        assert gb[P - 1] == 0.0                                           # no gate uses the parameter
        assert np.abs(g_ref).max() > 1e-3 and abs(clean[b] - e_ref) > 1e-6      # not vacuous
    assert off == g.size


# ---- d. device L-BFGS ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", list(NOISE))
def test_device_lbfgs_at_eleven_qubits(tq, noise):
    """The lock-step driver's only contact with more than 4 tiles per partial: a few iterations on one circuit; the
    returned f is the oracle's channel energy at the returned x, and no higher than at the start."""
    n = 11
    three, states, psi0, ham = _problem(n)
    p1, p2 = NOISE[noise]
    w, c = _grad_case(n)[0]
    levels = _n_blocks(n, c, p1, p2)
    eng = _engine(tq, n, psi0, ham, p1, p2, batched=levels + 2, grad=True)
    eng.set_circuit(_circ(tq, c))
    x, f, nfev, nit, status = eng.minimize_lbfgs(c[4], history=3, maxiter=4, maxfun=40)
    scale = _scale(ham)
    e0 = fo.energy(n, three[w], states[w], c[:4], c[4], ham, p1, p2)
    ex = fo.energy(n, three[w], states[w], c[:4], x, ham, p1, p2)
    clean = fo.energy(n, three[w], states[w], c[:4], x, ham, p1, p2, noiseless=True)
    print(f"L-BFGS n={n} p=({p1}, {p2}): (nfev, nit, status)=({nfev}, {nit}, {status}) f(x0)={e0:.8f} f={f:.8f} "
          f"|f - E(x)|={abs(f - ex):.2e} ({abs(f - ex) / (E_TOL * scale):.1e} of the bound)")
    assert abs(f - ex) <= E_TOL * scale, (f, ex)
    assert f <= e0 + E_TOL * scale and 1 <= nit <= 4 and nfev <= 40
    assert abs(eng.energy(c[4]) - e0) <= E_TOL * scale
    assert f <= eng.energy(c[4])
    assert abs(clean - ex) > 1e-6
