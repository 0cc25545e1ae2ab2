"""GPU: the RXX / RYY / RZZ gate kinds on every kernel path against the unmodified CPU oracle, through the expansion of
su4_helpers (pinned against the definition by test_su4_cpu.py).  Tolerances as in test_hip_parity.py: energies
1e-10 Ha, amplitudes 1e-12."""
import importlib

import numpy as np
import pytest

import vqe_oracle as vo
import su4_helpers as s4
from helpers import fermionic_hamiltonian, load_case, random_hamiltonian, random_state

pytestmark = pytest.mark.gpu

E_TOL = 1e-10
A_TOL = 1e-12


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _engine(tq, n, psi0, ham):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    return eng


def _check(tq, eng, psi0, g, hams, state=True):
    kind, q0, q1, pidx, th = g
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    psi = s4.run_circuit(psi0, kind, q0, q1, pidx, th)
    if state:
        da = np.abs(eng.get_state(th) - psi).max()
        print(f"n={eng.n_qubits} gates={kind.size}: max amplitude error {da:.2e}")
        assert da < A_TOL
    for ham in hams:
        eng.set_hamiltonian(*ham)
        de = abs(eng.energy(th) - vo.energy_pauli(psi, *ham))
        print(f"n={eng.n_qubits} gates={kind.size} terms={ham[0].size}: energy error {de:.2e}")
        assert de < E_TOL


# plain LDS kernels (n <= 9), register path (10..13), streaming path (14, 16)
@pytest.mark.parametrize("n,G", [(2, 14), (3, 24), (5, 60), (8, 120), (9, 90), (10, 80), (12, 100), (13, 50), (14, 40), (16, 24)])
def test_state_and_energy_parity(tq, n, G):
    rng = np.random.default_rng(6000 + n)
    psi0 = random_state(n, rng)
    g = s4.random_gates_su4(n, G, rng)
    assert {6, 7, 8} <= set(g[0].tolist())
    hams = [random_hamiltonian(n, 10 + 4 * n, rng), random_hamiltonian(n, 10 + 2 * n, rng, real=False)]
    if n >= 4:
        hams.append(fermionic_hamiltonian(n, n_hop=2 * n, n_quad=n, rng=rng, dressed=2))
    if n >= 14:
        # more X-mask groups than the tile planner's pass table takes (32 passes x 7 masks): the one-sweep-per-four-ops
        # circuit kernel and the plain reduction serve this handle, the tiled kernels the others
        many = random_hamiltonian(n, 300, rng)
        assert np.unique(many[0]).size > 32 * 7
        hams.append(many)
    eng = _engine(tq, n, psi0, hams[0])
    _check(tq, eng, psi0, g, hams)
    if n >= 14:      # the state as the fallback circuit kernel leaves it
        assert np.abs(eng.get_state(g[4]) - s4.run_circuit(psi0, *g)).max() < A_TOL
    # a batch of angles through the same compiled circuit
    kind, q0, q1, pidx, th = g
    eng.set_hamiltonian(*hams[0])
    ths = th[None, :] + rng.normal(size=(3, th.size))
    got = eng.energy_batch(ths)
    for i in range(3):
        assert abs(got[i] - s4.energy(psi0, kind, q0, q1, pidx, ths[i], hams[0])) < E_TOL
    eng.close()


@pytest.mark.parametrize("n", [5, 12, 14])
def test_circuit_of_only_rzz(tq, n):
    """No pair op at all: one layout, one tile pass, nothing to re-distribute."""
    rng = np.random.default_rng(6100 + n)
    psi0 = random_state(n, rng)
    G = 3 * n
    q0 = rng.integers(0, n, G)
    q1 = (q0 + 1 + rng.integers(0, n - 1, G)) % n
    g = (np.full(G, 8, np.int32), q0.astype(np.int32), q1.astype(np.int32), np.arange(G, dtype=np.int32),
         rng.uniform(-np.pi, np.pi, G))
    eng = _engine(tq, n, psi0, random_hamiltonian(n, 40, rng))
    _check(tq, eng, psi0, g, [random_hamiltonian(n, 40, rng), random_hamiltonian(n, 30, rng, real=False)])
    eng.close()


def test_register_path_many_layouts():
    """n = 12 keeps four register directions: thirty RXX / RYY on distinct pairs and no CNOT span all of GF(2)^12 minus
    one dimension (every mask has even weight), so the scheduler opens several layouts - and the composite masks are what
    it takes as directions."""
    import tensorrl_qas_amd as tq
    n = 12
    rng = np.random.default_rng(6200)
    psi0 = random_state(n, rng)
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
    rng.shuffle(pairs)
    kind, q0, q1 = [], [], []
    for i, (a, b) in enumerate(pairs[:30]):
        kind.append(6 + (i % 2)), q0.append(a), q1.append(b)
        if i % 5 == 4:
            kind.append(8), q0.append(b), q1.append(a)
    G = len(kind)
    g = (np.array(kind, np.int32), np.array(q0, np.int32), np.array(q1, np.int32), np.arange(G, dtype=np.int32),
         rng.uniform(-np.pi, np.pi, G))
    eng = _engine(tq, n, psi0, random_hamiltonian(n, 50, rng))
    _check(tq, eng, psi0, g, [random_hamiltonian(n, 50, rng), fermionic_hamiltonian(n, 20, 12, rng, dressed=2)])
    eng.close()


@pytest.mark.parametrize("n", [5, 9, 12, 13, 14])
def test_identities_without_the_oracle(tq, n):
    """RXX(a,b) = CNOT RX(a) CNOT and RZZ(a,b) = CNOT RZ(b) CNOT: the same engine, the two spellings, 1e-12."""
    rng = np.random.default_rng(6300 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 40, rng)
    kind, q0, q1, pidx, th = s4.random_gates_su4(n, 50, rng)
    keep = kind != 7
    kind, q0, q1 = kind[keep], q0[keep], q1[keep]
    pidx = np.where(kind > 0, np.cumsum(kind > 0) - 1, -1).astype(np.int32)
    th = th[:int((kind > 0).sum())]
    assert {6, 8} <= set(kind.tolist())
    eng = _engine(tq, n, psi0, ham)
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    e_new = eng.energy(th)
    k2, a2, b2, p2 = s4.expand(kind, q0, q1, pidx, th.size)
    assert k2.max() <= 3
    eng.set_circuit(tq.Circuit(k2, a2, b2, p2, th.size))
    e_old = eng.energy(th)
    print(f"n={n}: |E(one op) - E(CNOT R CNOT)| = {abs(e_new - e_old):.2e}")
    assert abs(e_new - e_old) <= 1e-12
    eng.close()


def _tie_free_su4(n, P, rng):
    """P rotations with distinct generators (two-qubit ones on distinct unordered pairs, one-qubit ones on distinct
    (qubit, axis)), CNOTs in between: COBYLA meets no exact ties (tests/test_configs_gpu.py: _tie_free_gates)."""
    two = [(a, b, k) for a in range(n) for b in range(a + 1, n) for k in (6, 7, 8)]
    one = [(q, -1, k) for q in range(n) for k in (1, 2, 3)]
    rng.shuffle(two), rng.shuffle(one)
    picks = two[:(P + 1) // 2] + one[:P // 2]
    rng.shuffle(picks)
    kind, q0, q1, pidx = [], [], [], []
    for j, (a, b, k) in enumerate(picks):
        if b >= 0 and rng.random() < 0.5:
            a, b = b, a
        kind.append(k), q0.append(a), q1.append(b), pidx.append(j)
        if rng.random() < 0.5:
            c = int(rng.integers(n))
            kind.append(0), q0.append(c), q1.append(int((c + 1 + rng.integers(n - 1)) % n)), pidx.append(-1)
    return tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)) + (rng.uniform(-np.pi, np.pi, P),)


@pytest.mark.parametrize("n", [4, 8, 10, 12])
def test_batch_energy_and_minimize(tq, n):
    """vqe_batch_load with circuits of different lengths that mix old and new kinds; the device COBYLA loop against the
    library's host COBYLA driven by ORACLE energies of the expanded circuit: the same optimum (1e-5, as
    test_device_cobyla_trajectory asks), the reported f is the oracle's energy at the reported x."""
    rng = np.random.default_rng(6400 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 30, rng)
    eng = _engine(tq, n, psi0, ham)
    raw = [_tie_free_su4(n, P, rng) for P in (5, 6, 8)]
    raw.append(s4.random_gates_su4(n, 3, rng))
    raw.append(tuple(np.zeros(0, np.int32) for _ in range(4)) + (np.zeros(0),))
    raw.append(s4.random_gates_su4(n, 40, rng))
    circs = [tq.Circuit(*g[:4], g[4].size) for g in raw]
    eng.batch_load(circs, [g[4] for g in raw])
    eng.batch_run_energy()
    _, f0, _ = eng.batch_fetch()
    for b, g in enumerate(raw):
        assert abs(f0[b] - s4.energy(psi0, *g, ham)) < E_TOL
    eng.batch_run_minimize(1.0, 1e-4, 1000)
    x, f, nfev = eng.batch_fetch()
    off = 0
    for b, g in enumerate(raw):
        P = g[4].size
        xb = x[off:off + P]
        off += P
        assert abs(s4.energy(psi0, *g[:4], xb, ham) - f[b]) < E_TOL
        assert f[b] <= f0[b] + 1e-12
        if b < 3:
            xh, fh, nh, _ = tq.HostCobyla(g[4], 1.0, 1e-4, 1000).minimize(lambda t: s4.energy(psi0, *g[:4], t, ham))
            print(f"n={n} P={P}: nfev device/host {nfev[b]}/{nh}, |df| = {abs(f[b] - fh):.2e}, |dx| = {np.abs(xb - xh).max():.2e}")
            assert abs(f[b] - fh) < 1e-5
    eng.close()


@pytest.mark.parametrize("n", [8, 12, 14])
def test_env_step_with_a_two_qubit_rotation_as_the_new_gate(tq, n):
    """vqe_batch_run_env_step: COBYLA sees the circuit without the new RXX / RYY / RZZ (its angle is not a variable and
    keeps its value), the optimum is rounded to float32, f is the oracle's energy of the full circuit.  n = 14: the
    host-built pre-action circuits of the streaming path."""
    rng = np.random.default_rng(6500 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 30, rng)
    eng = _engine(tq, n, psi0, ham)
    raw, new = [], []
    for b, k in enumerate((6, 7, 8, 6)):
        g = list(s4.random_gates_su4(n, 8 + 2 * b, rng))
        at = [0, g[0].size // 2, g[0].size - 1, g[0].size - 1][b]
        c = int(rng.integers(n))
        t = int((c + 1 + rng.integers(n - 1)) % n)
        g[0] = np.insert(g[0], at, k).astype(np.int32)
        g[1] = np.insert(g[1], at, c).astype(np.int32)
        g[2] = np.insert(g[2], at, t).astype(np.int32)
        g[3] = np.where(g[0] > 0, np.cumsum(g[0] > 0) - 1, -1).astype(np.int32)
        hole = int(g[3][at])
        g[4] = np.insert(g[4], hole, 0.25 if b == 3 else 0.0).astype(np.float32).astype(np.float64)
        raw.append(g), new.append(at)
    eng.batch_load([tq.Circuit(*g[:4], g[4].size) for g in raw], [g[4] for g in raw])
    eng.batch_set_new_gate(new)
    maxfun = 1000 if n <= 13 else 80
    eng.batch_run_env_step(1.0, 1e-4, maxfun)
    x, f, nfev = eng.batch_fetch()
    xopt = eng.batch_fetch_xopt()
    off = 0
    for b, (g, at) in enumerate(zip(raw, new)):
        kind, q0, q1, pidx, th = g
        P = th.size
        xb, xr = x[off:off + P], xopt[off:off + P]
        off += P
        hole = int(pidx[at])
        assert xb[hole] == th[hole] and xr[hole] == th[hole]
        assert np.array_equal(xb, xr.astype(np.float32).astype(np.float64))
        assert abs(s4.energy(psi0, kind, q0, q1, pidx, xb, ham) - f[b]) < E_TOL
        keep = np.ones(kind.size, bool)
        keep[at] = False
        sel = [j for j in range(P) if j != hole]
        pre = np.where(pidx > hole, pidx - 1, pidx)
        cost = lambda t: s4.energy(psi0, kind[keep], q0[keep], q1[keep], pre[keep], t, ham)
        assert cost(xr[sel]) <= cost(th[sel]) + 1e-12
        assert 1 <= nfev[b] <= maxfun
        if n <= 13:      # the fused launch stopped where COBYLA itself finds nothing better (test_env_step_semantics)
            _, fp, _, _ = tq.HostCobyla(xr[sel], 1e-3, 1e-4, 1000).minimize(cost)
            assert fp >= cost(xr[sel]) - 1e-5
    eng.close()


@pytest.mark.parametrize("n", [2, 5, 8, 10, 12, 13])
def test_grad_parity(tq, n):
    rng = np.random.default_rng(6600 + n)
    G = {2: 14, 5: 36, 8: 50, 10: 40, 12: 36, 13: 24}[n]
    g = s4.random_gates_su4(n, G, rng)
    kind, q0, q1, pidx, th = g
    assert {6, 7, 8} <= set(kind.tolist())
    psi0 = random_state(n, rng)
    hams = [random_hamiltonian(n, 6 + 2 * n, rng, real=False)]
    if n >= 4:
        hams.append(fermionic_hamiltonian(n, n_hop=2 * n, n_quad=n, rng=rng, dressed=2))
    for ham in hams:
        eng = _engine(tq, n, psi0, ham)
        eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
        e, gr = eng.energy_grad(th)
        g_ref = s4.shift_grad(psi0, kind, q0, q1, pidx, th, ham)
        scale = max(1.0, float(np.abs(ham[2]).sum()))
        print(f"n={n}: max gradient error {np.abs(gr - g_ref).max():.2e} (scale {scale:.1f})")
        assert np.abs(gr - g_ref).max() <= 1e-10 * scale
        assert abs(e - s4.energy(psi0, kind, q0, q1, pidx, th, ham)) <= 1e-10 * scale
        eng.close()


def test_grad_shared_parameters_and_term_shards(tq):
    n = 6
    rng = np.random.default_rng(6700)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 24, rng, real=False)
    # parameter 0 drives an RX on q3 and an RYY on (1, 4); parameter 1 an RZZ and an RXX; parameter 3 no gate
    kind = np.array([1, 0, 7, 8, 0, 6, 2, 7], np.int32)
    q0 = np.array([3, 1, 1, 0, 4, 2, 5, 5], np.int32)
    q1 = np.array([-1, 2, 4, 3, 0, 5, -1, 0], np.int32)
    pidx = np.array([0, -1, 0, 1, -1, 1, 2, 4], np.int32)
    th = np.array([0.7, -1.1, 2.0, 0.4, -0.3])
    circ = tq.Circuit(kind, q0, q1, pidx, 5)
    eng = _engine(tq, n, psi0, ham)
    eng.set_circuit(circ)
    e, g = eng.energy_grad(th)
    scale = max(1.0, float(np.abs(ham[2]).sum()))
    assert g[3] == 0.0
    assert np.abs(g - s4.shift_grad(psi0, kind, q0, q1, pidx, th, ham)).max() <= 1e-10 * scale
    h = 1e-5
    for j in (0, 1):      # the finite difference of the SHARED angle agrees with the sum over its gates
        tp, tm = th.copy(), th.copy()
        tp[j] += h
        tm[j] -= h
        fd = (s4.energy(psi0, kind, q0, q1, pidx, tp, ham) - s4.energy(psi0, kind, q0, q1, pidx, tm, ham)) / (2 * h)
        assert abs(g[j] - fd) < 1e-7 * scale
    n = 10
    kind, q0, q1, pidx, th = s4.random_gates_su4(n, 40, rng)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, n_hop=14, n_quad=8, rng=rng, dressed=2)
    circ = tq.Circuit(kind, q0, q1, pidx, th.size)
    parts = []
    for r in (None, 0, 1):
        eng = _engine(tq, n, psi0, ham)
        eng.set_circuit(circ)
        if r is not None:
            eng.set_term_shard(r, 2)
        parts.append(eng.energy_grad(th))
        eng.close()
    assert abs(parts[1][0] + parts[2][0] - parts[0][0]) <= 1e-12
    assert np.abs(parts[1][1] + parts[2][1] - parts[0][1]).max() <= 1e-12


def test_refusals(tq):
    n = 5
    rng = np.random.default_rng(6800)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 12, rng)
    g = s4.random_gates_su4(n, 20, rng)
    kind, q0, q1, pidx, th = g
    e_ref = s4.energy(psi0, *g, ham)
    eng = _engine(tq, n, psi0, ham)
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    eng.set_noise(0.01, 0.02, 1)
    eng.set_noise_mode(1)
    with pytest.raises(tq.VQEError, match="-22.*RXX"):
        eng.energy(th)
    with pytest.raises(tq.VQEError, match="-22"):
        eng.minimize_cobyla(th, 1.0, 1e-4, 50)
    eng.set_noise_mode(0)
    eng.set_noise(0.0, 0.0, 1)
    assert abs(eng.energy(th) - e_ref) < E_TOL      # the handle is still usable
    for k in (6, 7, 8):
        for a, b, p in ((1, 1, 0), (1, n, 0), (n, 1, 0), (-1, 2, 0), (0, -1, 0), (0, 1, 1), (0, 1, -1)):
            with pytest.raises(tq.VQEError, match="-22"):
                eng.set_circuit(tq.Circuit([k], [a], [b], [p], 1))
    with pytest.raises(tq.VQEError, match="-22.*unknown gate kind"):
        eng.set_circuit(tq.Circuit([9], [0], [1], [0], 1))
    # Pauli-trajectory noise behind the new gates is ordinary: at p = 0 the channels are identities
    k2 = np.concatenate([kind, [5, 4]]).astype(np.int32)
    eng.set_circuit(tq.Circuit(k2, np.concatenate([q0, [0, 2]]), np.concatenate([q1, [1, -1]]), np.concatenate([pidx, [-1, -1]]), th.size))
    assert abs(eng.energy(th) - e_ref) < E_TOL
    eng.close()


@pytest.mark.parametrize("n", [6, 11, 14])
def test_pauli_trajectory_noise_behind_the_new_gates(tq, n):
    """DEPOL1 / DEPOL2 records follow the new gates like any other.  With the draws of the C oracle's restated
    generator the noisy energies agree to 1e-10: an X or Y error ahead of a two-qubit rotation flips the sign bit
    c[q0] ^ c[q1] of its op (plain LDS, register and streaming path)."""
    import c_oracle as co
    rng = np.random.default_rng(6900 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 30, rng, real=False)
    base = s4.random_gates_su4(n, 30 if n < 14 else 14, rng)
    kind, q0, q1, pidx = [], [], [], []
    for k, a, b, p in zip(*base[:4]):
        kind += [int(k), 5 if b >= 0 else 4]; q0 += [int(a)] * 2; q1 += [int(b)] * 2; pidx += [int(p), -1]
    kind, q0, q1, pidx = (np.array(v, np.int32) for v in (kind, q0, q1, pidx))
    th = base[4]
    p1, p2, seed = 0.3, 0.6, 13572468
    eng = _engine(tq, n, psi0, ham)
    eng.set_noise(p1, p2, seed)
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    seen = set()
    n_eval = 8 if n < 14 else 3
    for e in range(n_eval):
        got = eng.energy(th)
        dr = co.noise_draws(seed, 0, e, kind, p1, p2)
        seen.update(dr.tolist())
        ref = vo.energy_pauli(s4.run_circuit(psi0, kind, q0, q1, pidx, th, dr), *ham)
        assert abs(got - ref) < E_TOL, (e, got, ref)
    assert len(seen) > 4
    got = eng.energy_batch(np.tile(th, (3, 1)))
    for b in range(3):
        dr = co.noise_draws(seed, b, n_eval, kind, p1, p2)
        assert abs(got[b] - vo.energy_pauli(s4.run_circuit(psi0, kind, q0, q1, pidx, th, dr), *ham)) < E_TOL
    dr = co.noise_draws(seed, 0, n_eval + 1, kind, p1, p2)
    assert np.abs(eng.get_state(th) - s4.run_circuit(psi0, kind, q0, q1, pidx, th, dr)).max() < A_TOL
    eng.close()


def test_su4_seam_on_the_golden_h2o_hamiltonian(tq):
    import torch
    su4 = importlib.import_module("tensorrl_qas_amd.environments.VQAs.VQE_qulacs_su4")
    d = load_case("H2O_8q")
    n = d["n"]
    xs, zs = tq.hamiltonian.masks_from_strings(d["paulis"], n)
    obs = tq.hamiltonian.PauliHamiltonian(n, xs, zs, d["weights"])
    rng = np.random.default_rng(7000)
    L = 3
    state = np.zeros((L, 6 * n + 6, n), np.float32)
    for l in range(L):
        for blk in range(3):
            for _ in range(3):
                t = int(rng.integers(n))
                c = int((t + 1 + rng.integers(n - 1)) % n)
                state[l, blk * n + t, c] = 1
                state[l, 3 * n + 3 + blk * n + t, c] = rng.uniform(-np.pi, np.pi)
        for _ in range(4):
            a, q = int(rng.integers(3)), int(rng.integers(n))
            state[l, 3 * n + a, q] = 1
            state[l, 6 * n + 3 + a, q] = rng.uniform(-np.pi, np.pi)
    circ = su4.Parametric_Circuit(n).construct_ansatz(torch.from_numpy(state))
    assert {1, 2, 3, 6, 7, 8} >= set(circ.kind.tolist()) and {6, 7, 8} <= set(circ.kind.tolist())
    psi0 = np.zeros(1 << n, np.complex128)
    psi0[0] = 1
    ham = (xs, zs, d["weights"])
    e = su4.get_exp_val(n, circ, obs)
    assert abs(e - s4.energy(psi0, circ.kind, circ.q0, circ.q1, circ.pidx, circ.angles, ham)) < E_TOL
    ang = rng.uniform(-np.pi, np.pi, circ.n_params)
    e2 = su4.get_energy_qulacs(ang, obs, circ, n, 0)
    assert abs(e2 - s4.energy(psi0, circ.kind, circ.q0, circ.q1, circ.pidx, ang, ham)) < E_TOL
    some = [0, circ.n_params - 1]
    e3 = su4.get_energy_qulacs([0.5, -0.5], obs, circ, n, 0, which_angles=some)
    ang[some] = [0.5, -0.5]
    assert abs(e3 - s4.energy(psi0, circ.kind, circ.q0, circ.q1, circ.pidx, ang, ham)) < E_TOL
