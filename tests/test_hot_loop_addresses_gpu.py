"""GPU: the address and wait bookkeeping of the env-step kernel's hot loops - results against the oracle where it can
go wrong.

(a) Unit loop (unit_energy): stepped offsets into arrays that end with two look-ahead trips, arithmetic of a unit
    started as its own two LDS reads arrive.  Number-conserving Hamiltonians held as exactly k = 1, 4, 5, 11, 12, 13
    units before padding (every residue of the trip of 4 and of the turn of 12; the Hamiltonians of
    tests/test_unit_padding_cpu.py), at 8 qubits (one wave), 10 and 12 (register path): energies of random circuits
    against the oracle to 1e-10, two runs bit for bit.
(b) Register path (run_ops_reg, reg_energy): the LDS addresses of the re-layouts, of the final scatter and of the state
    reads.  Circuits that alternate RX / RY blocks between two disjoint sets of as many qubits as the size keeps
    register directions, with CNOTs between the blocks: every block after the first opens a new layout (counted
    here with the scheduler's rule).  n = 10, 11, 12, 13: state to 1e-12, energy to 1e-10.  (Absolute LDS addresses on
    this path were measured and not adopted; the circuits stay as the check of any later attempt.)
(c) One environment step of 4 environments at 10 qubits, maxfun 60, by the reference path of the env-step test of
    tests/test_lds_sizes_gpu.py: every traced value is the oracle's energy at the traced point, the host COBYLA told
    the device's values proposes the same points, float32 round trip, energy of the full circuit, and the same nfev
    in a second run."""
import numpy as np
import pytest

import lds_cases as lc
from helpers import fermionic_hamiltonian, random_gates, random_state

pytestmark = pytest.mark.gpu

UNIT_COUNTS = (1, 4, 5, 11, 12, 13)


def octet_hamiltonian(n, k, seed):
    """Identity + Z + ZZ terms and k double-excitation octets: k units (tests/test_unit_padding_cpu.py counts them)."""
    return fermionic_hamiltonian(n, 0, k, np.random.default_rng(seed), 0)


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _engine(tq, n, psi0, ham):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    return eng


# ---- (a) unit loop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 10, 12])
@pytest.mark.parametrize("k", UNIT_COUNTS)
def test_unit_loop_by_unit_count(tq, n, k):
    rng = np.random.default_rng(8200 + 16 * n + k)
    psi0 = random_state(n, rng)
    ham = octet_hamiltonian(n, k, 8100 + 16 * n + k)
    eng = _engine(tq, n, psi0, ham)
    assert eng.hamiltonian_layout()["units"] == 12 * ((k + 11) // 12)      # the loop bound: whole turns, no look-ahead
    worst = 0.0
    for c in range(3):
        kind, q0, q1, pidx, th = random_gates(n, 16 + 4 * c, rng)
        eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
        ths = np.concatenate([th[None, :], th[None, :] + rng.normal(size=(1, th.size))])
        got = eng.energy_batch(ths)
        again = eng.energy_batch(ths)
        assert np.array_equal(got, again)
        ref = np.array([lc.oracle_energy(n, psi0, (kind, q0, q1, pidx), t, ham) for t in ths])
        worst = max(worst, float(np.abs(got - ref).max()))
    print(f"n={n} k={k}: worst |dE| = {worst:.2e}")
    assert worst <= 1e-10
    eng.close()


# ---- (b) register path ----------------------------------------------------------------------------------------------
def _register_directions(n):
    return n - (9 if n >= 13 else 8)       # Geo<N>: 2^R amplitudes per thread on 256 (512 at 13 qubits) threads


def relayout_circuit(n, blocks, rng):
    """RX / RY (and an RZ) on each qubit of S1 = {0..R-1}, then of S2 = {R..2R-1}, S1 again, ...; between two blocks a
    CNOT from a qubit of the block just done into the other set and one with a qubit of neither set."""
    R = _register_directions(n)
    sets = (list(range(R)), list(range(R, 2 * R)))
    rest = list(range(2 * R, n))
    kind, q0, q1, pidx, th = [], [], [], [], []

    def rot(k, q):
        kind.append(k), q0.append(q), q1.append(-1), pidx.append(len(th)), th.append(float(rng.uniform(-np.pi, np.pi)))

    for b in range(blocks):
        s, other = sets[b % 2], sets[(b + 1) % 2]
        for i, q in enumerate(s):
            rot(1 + (i + b) % 2, q)
            rot(3, q)
        if b + 1 < blocks:
            kind.append(0), q0.append(s[b % R]), q1.append(other[(b + 1) % R]), pidx.append(-1)
            kind.append(0), q0.append(rest[b % len(rest)]), q1.append(s[0]), pidx.append(-1)
    return tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)) + (np.array(th, np.float64),)


def count_relayouts(n, kind, q0, q1):
    """The rule of schedule_ops (csrc/vqe_reg.h).  CNOTs are folded into the affine index map i = A p ^ c: a rotation
    on logical qubit q exchanges amplitudes whose physical indices differ by column q of A^-1, and CNOT(c, t) adds
    column t to column c.  A layout holds the span of the first R independent pair masks from where it is opened; a
    pair op whose mask lies outside the span opens the next."""
    R = _register_directions(n)
    col = [1 << q for q in range(n)]
    masks = []                       # pair masks in execution order
    for k, a, b in zip(kind, q0, q1):
        if k == 0:
            col[a] ^= col[b]
        elif k in (1, 2):
            masks.append(col[a])

    def reduce(basis, v):
        for e in basis:
            v = min(v, v ^ e)
        return v

    def open_layout(start):
        basis = []
        for m in masks[start:]:
            if len(basis) == R:
                break
            r = reduce(basis, m)
            if r:
                basis.append(r)
                basis.sort(reverse=True)
        return basis

    basis, count = open_layout(0), 0
    for i, m in enumerate(masks):
        if reduce(basis, m):
            basis = open_layout(i)
            count += 1
    return count


@pytest.mark.parametrize("n", [10, 11, 12, 13])
def test_register_path_relayouts(tq, n):
    rng = np.random.default_rng(8300 + n)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, 2 * n, 2 * n, rng, 2)      # units, class groups and the bank swizzle
    kind, q0, q1, pidx, th = relayout_circuit(n, 5, rng)
    assert count_relayouts(n, kind, q0, q1) >= 3
    eng = _engine(tq, n, psi0, ham)
    assert eng.hamiltonian_layout()["units"] > 0
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    ref_psi = lc.run_circuit(n, psi0, kind, q0, q1, pidx, th)
    d_psi = float(np.abs(eng.get_state(th) - ref_psi).max())
    d_e = abs(eng.energy(th) - lc.energy_of(n, ref_psi, ham))
    print(f"n={n}: {count_relayouts(n, kind, q0, q1)} re-layouts, max |dpsi| = {d_psi:.2e}, |dE| = {d_e:.2e}")
    assert d_psi <= 1e-12
    assert d_e <= 1e-10
    eng.close()


# ---- (c) one environment step ---------------------------------------------------------------------------------------
def _pre_action(gates, P, ng):
    """The circuit the optimiser sees when gate ``ng`` (-1: none) is the new one -> (gates, variables, hole or -1)"""
    kind, q0, q1, pidx = gates
    keep = np.ones(kind.size, bool)
    hole = -1
    if ng >= 0:
        keep[ng] = False
        if kind[ng] != 0:
            hole = int(pidx[ng])
    sel = [j for j in range(P) if j != hole]
    pp = np.where(pidx[keep] > hole, pidx[keep] - 1, pidx[keep]) if hole >= 0 else pidx[keep]
    return (kind[keep], q0[keep], q1[keep], pp), sel, hole


def test_env_step_four_environments(tq):
    n, maxfun, P = 10, 60, 10
    psi0, ham = lc.inputs(n)

    def build(b, j):
        gates, th = lc.cobyla_circuit(n, P, 8400 + b + 100000 * j)
        th = th.astype(np.float32).astype(np.float64)
        kind = gates[0]
        rot, cn = np.nonzero(kind != 0)[0], np.nonzero(kind == 0)[0]
        ng = [int(rot[rot.size // 2]), -1, int(cn[cn.size // 2]) if cn.size else -1, int(rot[-1])][b]
        if ng >= 0 and kind[ng] != 0:
            th[gates[3][ng]] = 0.0                    # a new rotation enters with theta = 0
        pre, sel, _ = _pre_action(gates, th.size, ng)
        return (gates, th, ng), (n, pre, th[sel], maxfun, None, None)

    cases = [lc.first_decided(lambda j, b=b: build(b, j), f"hot-loop env-step circuit {b}") for b in range(4)]
    circuits = [(g, th) for g, th, _ in cases]
    new = [ng for _, _, ng in cases]
    eng = lc.engine(tq, n)
    assert eng.hamiltonian_layout()["units"] > 0
    x, xraw, f, nfev, traces = lc.traced_minimize(eng, tq, circuits, maxfun, None, new)
    off = 0
    for b, (gates, th) in enumerate(circuits):
        xb, xr = x[off:off + P], xraw[off:off + P]
        off += P
        pre, sel, hole = _pre_action(gates, P, new[b])
        ft, xt = traces[b]
        lc.check_trace(tq, n, pre, th[sel], ft, xt[:, :len(sel)], int(nfev[b]), maxfun)
        if hole >= 0:
            assert xb[hole] == th[hole] == 0.0
        assert np.array_equal(xb, xr.astype(np.float32).astype(np.float64))
        assert abs(f[b] - lc.oracle_energy(n, psi0, gates, xb, ham)) < lc.E_TOL
    # the same launch again, untraced: energies, points and evaluation counts bit for bit
    eng.batch_load([tq.Circuit(*g, th.size) for g, th in circuits], [th for _, th in circuits])
    eng.batch_set_new_gate(new)
    eng.batch_run_env_step(1.0, 1e-4, maxfun)
    x2, f2, nfev2 = eng.batch_fetch()
    assert np.array_equal(x, x2) and np.array_equal(f, f2) and np.array_equal(nfev, nfev2)
    eng.close()
