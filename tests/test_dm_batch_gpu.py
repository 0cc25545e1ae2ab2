"""GPU: the batched lock-step form of the exact channel mode (vqe_set_dm_batched: csrc/vqe_dm_batch.h) -
energies against the oracle's channel, independence of a circuit's bits from the batch around it, window bits above the
ket half, base offsets beyond 4 GiB, the device COBYLA pinned against the host build driven by this path's own energies,
early finishers, the unchanged default, the refusals and the environments' ``noise_channel="exact"``.
The serial path's tests are tests/test_dm_gpu.py; the plan / fill split is checked on the CPU (tests/test_dm_plan_cpu.py)."""
import functools

import numpy as np
import pytest

import vqe_oracle as vo
from dm_batch_cases import gate_list, mixed_batch, noisy
from helpers import random_gates, random_hamiltonian, random_state

pytestmark = pytest.mark.gpu
E_TOL = 1e-10


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _engine(tq, n, psi0, ham, p1, p2, batched=-1, seed=11):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(p1, p2, seed)
    eng.set_noise_mode(1)
    if batched is not None:
        eng.set_dm_batched(batched)
    return eng


def _circ(tq, c):
    return tq.Circuit(c[0], c[1], c[2], c[3], c[4].size)


def _energies(tq, eng, circuits):
    eng.batch_load([_circ(tq, c) for c in circuits], [c[4] for c in circuits])
    eng.batch_run_energy()
    return eng.batch_fetch(want_x=False)[1].copy()


def _oracle(psi0, ham, c, theta, p1, p2):
    return vo.energy_dm(vo.run_circuit_dm(psi0, c[0], c[1], c[2], c[3], theta, p1, p2), *ham)


def _n_blocks(tq, n, c, p1, p2):
    import ctypes as C
    from tensorrl_qas_amd import _lib
    nb = C.c_int32()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib.c_i32p)
    th = np.ascontiguousarray(c[4] if c[4].size else np.zeros(1))
    assert _lib.load().vqe_dm_plan(n, len(c[0]), i32(c[0]), i32(c[1]), i32(c[2]), i32(c[3]), th.ctypes.data_as(_lib.c_f64p),
                                   p1, p2, 0, C.byref(nb), None, None) == 0
    return nb.value


CASES = [(2, 8, 0.2, 0.3, 0), (3, 14, 0.1, 0.25, 1), (4, 20, 0.3, 0.1, 2), (5, 30, 0.05, 0.2, 3), (6, 40, 0.01, 0.05, 4),
         (8, 40, 0.01, 0.05, 5)]


@functools.lru_cache(maxsize=None)
def _case(n, G, p1, p2, seed):
    """(psi0, ham, circuits, oracle energies) of one case: made once, shared, never modified"""
    rng = np.random.default_rng(8100 + seed)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 30, rng, real=False)
    circuits = mixed_batch(n, G, rng)
    ref = np.array([_oracle(psi0, ham, c, c[4], p1, p2) for c in circuits])
    return psi0, ham, circuits, ref


@pytest.mark.parametrize("n,G,p1,p2,seed", CASES)
def test_batched_energies_match_the_oracle(tq, n, G, p1, p2, seed):
    psi0, ham, circuits, ref = _case(n, G, p1, p2, seed)
    assert len(circuits[2][0]) == 0 and not np.any(circuits[3][0] >= 4)      # one without gates, one without noise gates
    assert len({len(c[0]) for c in circuits}) == 5
    eng = _engine(tq, n, psi0, ham, p1, p2)
    got = _energies(tq, eng, circuits)
    print(np.abs(got - ref))
    assert np.abs(got - ref).max() < E_TOL, (got, ref)
    info = eng.dm_batch_info()
    assert info["resident"] == 5 and info["chunks"] == 1 and info["evaluations"] == 1
    assert abs(got[2] - vo.energy_pauli(psi0, *ham)) < E_TOL                  # zero gates: the energy of the initial state
    # the single-circuit entry points take the same path
    eng.set_circuit(_circ(tq, circuits[0]))
    th = circuits[0][4]
    assert eng.energy(th) == got[0]
    assert np.array_equal(eng.energy_batch(np.stack([th, th])), got[[0, 0]])


def test_batched_energies_at_ten_qubits(tq):
    n, p1, p2 = 10, 0.01, 0.05
    rng = np.random.default_rng(8110)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 30, rng, real=False)
    circuits = [noisy(random_gates(n, G, rng)) for G in (12, 3, 5)]
    got = _energies(tq, _engine(tq, n, psi0, ham, p1, p2), circuits)
    ref = np.array([_oracle(psi0, ham, c, c[4], p1, p2) for c in circuits])
    print(np.abs(got - ref))
    assert np.abs(got - ref).max() < E_TOL, (got, ref)


def test_energy_is_independent_of_batch_position_and_chunking(tq):
    n, G, p1, p2, seed = CASES[3]
    psi0, ham, circuits, ref = _case(n, G, p1, p2, seed)
    levels = max(_n_blocks(tq, n, c, p1, p2) for c in circuits)
    base = None
    for R in (1, 2, -1):
        eng = _engine(tq, n, psi0, ham, p1, p2, batched=R)
        got = _energies(tq, eng, circuits)
        info = eng.dm_batch_info()
        r = 5 if R < 0 else R
        assert info == {"resident": r, "chunks": -(-5 // r), "evaluations": 1, "levels": levels}, info
        base = got if base is None else base
        assert np.array_equal(got, base), R
        assert np.array_equal(_energies(tq, eng, circuits[::-1])[::-1], base), R
    assert np.abs(base - ref).max() < E_TOL
    eng = _engine(tq, n, psi0, ham, p1, p2)
    alone = np.array([_energies(tq, eng, [c])[0] for c in circuits])
    assert np.array_equal(alone, base)


def test_high_window_bits(tq):
    """n = 12: blocks on (10, 11) and (0, 11) while the block on (4, 5) stays open beside them; p = 0, so the channel
    energy is the state-vector one."""
    n = 12
    rng = np.random.default_rng(8120)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 30, rng, real=False)
    a = gate_list([(0, 4, 5, None), (1, 10, -1, 0.7), (0, 10, 11, None), (3, 11, -1, -1.1), (0, 11, 0, None), (2, 0, -1, 0.2),
                   (1, 5, -1, 2.0), (0, 0, 11, None)])
    b = gate_list([(2, 4, -1, 0.4), (0, 5, 4, None), (0, 11, 10, None), (1, 11, -1, 1.3), (2, 10, -1, -0.6), (0, 0, 11, None),
                   (3, 0, -1, 0.9), (3, 4, -1, -2.2)])
    windows = lambda c: {tuple(sorted(w)) for w in zip(c[1][c[0] == 0], c[2][c[0] == 0])}
    assert {(10, 11), (0, 11), (4, 5)} <= windows(a) and {(10, 11), (0, 11), (4, 5)} <= windows(b)
    got = _energies(tq, _engine(tq, n, psi0, ham, 0.0, 0.0), [noisy(a), noisy(b)])
    ref = np.array([vo.energy_pauli(vo.run_circuit(psi0, *c), *ham) for c in (a, b)])
    print(np.abs(got - ref))
    assert np.abs(got - ref).max() < E_TOL, (got, ref)


def test_base_offsets_beyond_4_gib(tq):
    """260 density matrices of 10 qubits resident at once (4.06 GiB): circuit 256 starts at byte 2^32."""
    n, B, p1, p2 = 10, 260, 0.01, 0.05
    rng = np.random.default_rng(8130)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 20, rng, real=False)
    circuits = [noisy(random_gates(n, 4, rng)) for _ in range(B)]
    eng = _engine(tq, n, psi0, ham, p1, p2, batched=B)
    got = _energies(tq, eng, circuits)
    assert eng.dm_batch_info()["resident"] == B and eng.dm_batch_info()["chunks"] == 1
    for b in (0, 128, 259):
        ref = _oracle(psi0, ham, circuits[b], circuits[b][4], p1, p2)
        assert abs(got[b] - ref) < E_TOL, (b, got[b], ref)
    one = _engine(tq, n, psi0, ham, p1, p2, batched=1)
    alone = np.array([_energies(tq, one, [c])[0] for c in circuits])
    assert np.array_equal(alone, got), np.flatnonzero(alone != got)


# ---- COBYLA on the device ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _opt_case():
    """n = 4, six circuits of 8-12 gates (+ channels): [3] has no parameters, the last unitary gate of [4] is a CNOT;
    angles are float32 values (an env-step starts from the state tensor)."""
    n = 4
    rng = np.random.default_rng(8140)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 25, rng)
    bases = [random_gates(n, G, rng, p_cnot=0.3) for G in (8, 12, 9)]
    bases.append(random_gates(n, 8, rng, p_cnot=1.0))
    k, a, b, p, th = random_gates(n, 9, rng, p_cnot=0.3)
    bases.append((np.append(k, 0).astype(np.int32), np.append(a, 1).astype(np.int32), np.append(b, 3).astype(np.int32),
                  np.append(p, -1).astype(np.int32), th))
    bases.append(random_gates(n, 11, rng, p_cnot=0.3))
    circuits = []
    for base in bases:
        c = noisy(base)
        circuits.append(c[:4] + (c[4].astype(np.float32).astype(np.float64),))
    assert circuits[3][4].size == 0 and all(8 <= len(c[0]) // 2 <= 12 for c in circuits)
    return n, psi0, ham, circuits, 0.02, 0.08


def _host_cobyla_on_this_path(tq, eng1, psi0, ham, c, x0, p1, p2, maxfun):
    """The library's host COBYLA driven by the batched path's own energies (second handle); the oracle checks every
    energy on the way.  -> (x, f, nfev)"""
    worst = [0.0]

    def cost(t):
        e = _energies(tq, eng1, [c[:4] + (np.asarray(t, np.float64),)])[0]
        worst[0] = max(worst[0], abs(e - _oracle(psi0, ham, c, t, p1, p2)))
        return e

    if x0.size == 0:
        return x0, cost(x0), 1
    x, f, nfev, _ = tq.HostCobyla(x0, 1.0, 1e-4, maxfun).minimize(cost)
    assert worst[0] < E_TOL
    return x, f, nfev


def test_device_cobyla_minimize(tq):
    """dm_batch_info "evaluations" after a minimisation: the largest nfev of the batch."""
    n, psi0, ham, circuits, p1, p2 = _opt_case()
    maxfun = 60
    eng = _engine(tq, n, psi0, ham, p1, p2, batched=4)
    eng.batch_load([_circ(tq, c) for c in circuits], [c[4] for c in circuits])
    eng.batch_run_minimize(1.0, 1e-4, maxfun)
    xs, fs, nf = eng.batch_fetch()
    assert np.array_equal(xs, eng.batch_fetch_xopt())
    info = eng.dm_batch_info()
    assert info["resident"] == 4 and info["chunks"] == 2 and info["evaluations"] == nf.max(), (info, nf)
    assert eng.last_kernel_ms() > 0.0
    eng1 = _engine(tq, n, psi0, ham, p1, p2)
    off = 0
    for b, c in enumerate(circuits):
        P = c[4].size
        x = xs[off:off + P]
        assert abs(fs[b] - _oracle(psi0, ham, c, x, p1, p2)) < E_TOL, b
        xh, fh, nh = _host_cobyla_on_this_path(tq, eng1, psi0, ham, c, c[4], p1, p2, maxfun)
        assert nf[b] == nh and np.array_equal(x, xh) and fs[b] == fh, (b, nf[b], nh)
        off += P
    assert nf[3] == 1 and nf.max() == maxfun
    # the single-circuit entry point takes the same path
    eng.set_circuit(_circ(tq, circuits[0]))
    x0, f0, n0 = eng.minimize_cobyla(circuits[0][4], 1.0, 1e-4, maxfun)
    P0 = circuits[0][4].size
    assert n0 == nf[0] and f0 == fs[0] and np.array_equal(x0, xs[:P0])


def test_device_cobyla_env_step(tq):
    """dm_batch_info "evaluations" after an env-step: the largest nfev of the batch + 1 for the evaluation of the full
    circuits at the float32-rounded optimum."""
    n, psi0, ham, circuits, p1, p2 = _opt_case()
    maxfun = 60
    new, thetas = [], []
    for c in circuits:
        kind, pidx, th = c[0], c[3], c[4].copy()
        g = int(np.flatnonzero(kind < 4)[-1])
        if kind[g] != 0:
            th[pidx[g]] = 0.0                       # the new rotation enters with angle 0
        new.append(g), thetas.append(th)
    assert circuits[4][0][new[4]] == 0              # one circuit's new gate is a CNOT
    eng = _engine(tq, n, psi0, ham, p1, p2, batched=4)
    eng.batch_load([_circ(tq, c) for c in circuits], thetas)
    eng.batch_set_new_gate(new)
    eng.batch_run_env_step(1.0, 1e-4, maxfun)
    xs, fs, nf = eng.batch_fetch()
    xr = eng.batch_fetch_xopt()
    assert np.array_equal(xs, xr.astype(np.float32).astype(np.float64))
    info = eng.dm_batch_info()
    assert info["evaluations"] == nf.max() + 1 and info["chunks"] == 2, (info, nf)
    eng1 = _engine(tq, n, psi0, ham, p1, p2)
    off = 0
    for b, (c, th, g) in enumerate(zip(circuits, thetas, new)):
        kind, q0, q1, pidx = c[:4]
        P = th.size
        x = xs[off:off + P]
        assert abs(fs[b] - _oracle(psi0, ham, c, x, p1, p2)) < E_TOL, b
        keep = np.ones(kind.size, bool)
        keep[g:g + 2] = False                       # the new gate and the channel behind it
        hole = int(pidx[g]) if kind[g] != 0 else -1
        sel = [j for j in range(P) if j != hole]
        pp = np.where(pidx[keep] > hole, pidx[keep] - 1, pidx[keep]) if hole >= 0 else pidx[keep]
        pre = (kind[keep], q0[keep], q1[keep], pp.astype(np.int32))
        xh, fh, nh = _host_cobyla_on_this_path(tq, eng1, psi0, ham, pre, th[sel], p1, p2, maxfun)
        assert nf[b] == nh and np.array_equal(xr[off:off + P][sel], xh) and (hole < 0 or x[hole] == 0.0), (b, nf[b], nh)
        off += P


def test_early_finishers_are_left_alone(tq):
    """One circuit starts at its optimum and stops while another still works towards maxfun: what the early one returns
    is what it returns when it runs alone (its evaluations stop, its result is not touched by the later iterations)."""
    n, psi0, ham, circuits, p1, p2 = _opt_case()
    maxfun = 70
    solo = _engine(tq, n, psi0, ham, p1, p2)
    early = circuits[0]
    solo.set_circuit(_circ(tq, early))
    x_opt, _, _ = solo.minimize_cobyla(early[4], 1.0, 1e-4, 2000)
    solo.batch_load([_circ(tq, early)], [x_opt])
    solo.batch_run_minimize(0.01, 1e-4, maxfun)
    xa, fa, na = solo.batch_fetch()
    eng = _engine(tq, n, psi0, ham, p1, p2, batched=4)
    batch = [circuits[1], early, circuits[5], circuits[3]]
    eng.batch_load([_circ(tq, c) for c in batch], [circuits[1][4], x_opt, circuits[5][4], circuits[3][4]])
    eng.batch_run_minimize(0.01, 1e-4, maxfun)
    xs, fs, nf = eng.batch_fetch()
    print(nf, na)
    assert nf[0] == maxfun and nf[1] < maxfun - 16, nf          # many lock-step iterations apart (two polls of the host at least)
    o = circuits[1][4].size
    assert nf[1] == na[0] and fs[1] == fa[0] and np.array_equal(xs[o:o + early[4].size], xa)
    assert abs(fs[1] - _oracle(psi0, ham, early, xa, p1, p2)) < E_TOL
    assert eng.dm_batch_info()["evaluations"] == maxfun


def test_default_is_the_serial_path(tq):
    n, G, p1, p2, seed = CASES[2]
    psi0, ham, circuits, ref = _case(n, G, p1, p2, seed)
    single = _engine(tq, n, psi0, ham, p1, p2, batched=None)
    want = []
    for c in circuits:
        single.set_circuit(_circ(tq, c))
        want.append(single.energy(c[4]))
    zeros = {"resident": 0, "chunks": 0, "evaluations": 0, "levels": 0}
    for batched in (None, 0):
        eng = _engine(tq, n, psi0, ham, p1, p2, batched=batched)
        assert eng.dm_batch_info() == zeros
        assert np.array_equal(_energies(tq, eng, circuits), np.array(want))
        assert eng.dm_batch_info() == zeros
    eng.set_dm_batched(2)                           # on, then off again: the serial path and its bits
    assert np.abs(_energies(tq, eng, circuits) - ref).max() < E_TOL and eng.dm_batch_info()["chunks"] == 3
    eng.set_dm_batched(0)
    assert np.array_equal(_energies(tq, eng, circuits), np.array(want)) and eng.dm_batch_info() == zeros


def test_refusals_and_term_shards(tq):
    n, p1, p2 = 5, 0.1, 0.2
    rng = np.random.default_rng(8177)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 40, rng, real=False)
    c = noisy(random_gates(n, 16, rng))
    full = _oracle(psi0, ham, c, c[4], p1, p2)
    tot = 0.0
    for r in range(3):
        eng = _engine(tq, n, psi0, ham, p1, p2)
        eng.set_term_shard(r, 3)
        tot += _energies(tq, eng, [c, c])[1]
        assert eng.dm_batch_info()["evaluations"] == 1
    assert abs(tot - full) < E_TOL
    # optimising on a term-sharded handle: VQE_ESTATE, nothing launched (the energies of the last run stay)
    before = eng.batch_fetch(want_x=False)[1].copy()
    with pytest.raises(tq.VQEError, match="error -1:"):
        eng.batch_run_minimize(1.0, 1e-4, 20)
    with pytest.raises(tq.VQEError, match="error -1:"):
        eng.batch_run_env_step(1.0, 1e-4, 20)
    assert np.array_equal(eng.batch_fetch(want_x=False)[1], before)
    # an RXX gate: VQE_EINVAL
    eng = _engine(tq, n, psi0, ham, p1, p2)
    rxx = (np.array([6], np.int32), np.array([0], np.int32), np.array([1], np.int32), np.array([0], np.int32), np.array([0.3]))
    eng.batch_load([_circ(tq, c), _circ(tq, rxx)], [c[4], rxx[4]])
    for run in (eng.batch_run_energy, lambda: eng.batch_run_minimize(1.0, 1e-4, 20), lambda: eng.batch_run_env_step(1.0, 1e-4, 20)):
        with pytest.raises(tq.VQEError, match="error -22:.*RXX"):
            run()
    assert eng.dm_batch_info() == {"resident": 0, "chunks": 0, "evaluations": 0, "levels": 0}
    # an amplitude shard is refused at n <= 13 as before, with the switch on
    with pytest.raises(tq.VQEError, match="error -1:"):
        eng.set_amplitude_shard(0, 2)
    # n = 14: the switch is accepted, the mode is not
    e14 = tq.VQEEngine(14)
    e14.set_dm_batched(-1)
    with pytest.raises(tq.VQEError, match="error -22:"):
        e14.set_noise_mode(1)
    with pytest.raises(tq.VQEError, match="error -22:"):
        eng.set_dm_batched(-2)


# ---- environments -------------------------------------------------------------------------------------------------

def test_vec_env_exact_channel(tmp_path_factory):
    """VecCircuitEnv(..., noise_channel="exact"): both host loops drive vqe_batch_run_env_step on the batched path -
    identical observations, rewards, dones, energies and nfev, and every reported energy is the oracle's channel energy
    of that environment's circuit at its reported angles."""
    import torch
    from helpers import load_case, make_data_root, oracle_init_state, reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv as Noiseless
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv as cls
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    data_root = make_data_root(str(tmp_path_factory.mktemp("dmrg-to-qc")))
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2_noise", data_root)
    conf["non_local_opt"]["global_iters"] = 40
    dev = torch.device("cuda:0")
    B = 4
    vn = VecCircuitEnv(cls, conf, dev, B, seed=4, native=True, noise_channel="exact")
    vp = VecCircuitEnv(cls, conf, dev, B, seed=4, native=False, noise_channel="exact")
    assert vn.native and not vp.native
    assert torch.equal(vn.reset(), vp.reset())
    case = load_case("H2O_8q")
    n = vp.num_qubits
    psi0 = oracle_init_state(case)
    xs, zs = vo.pauli_masks(case["paulis"], n, reverse=False)
    table = vp.envs[0]._actions_table
    # per environment: CNOTs and rotations that share qubits, so that the channels matter
    script = [[0, 56 + 1 * 3 + 1, 7 + 1], [56 + 0 * 3 + 0, 1, 56 + 2 * 3 + 2], [8, 56 + 3 * 3 + 1, 56 + 1 * 3 + 0], [56 + 5 * 3 + 2, 56 + 5 * 3 + 0, 40]]
    for t in range(3):
        acts = [table[script[b][t]] for b in range(B)]
        on, rn, dn = vn.step(acts)
        op, rp, dp = vp.step(acts)
        assert torch.equal(on, op) and torch.equal(rn, rp) and dn == dp, t
        assert vn.engine.dm_batch_info()["evaluations"] >= 2 and vn.engine.dm_batch_info() == vp.engine.dm_batch_info()
        for b in range(B):
            e, w = vp.envs[b], vn.envs[b]
            assert (w.energy, w.nfev) == (e.energy, e.nfev) and 1 <= e.nfev <= 40
            assert torch.equal(w.state, e.state)
            k, a, q, p, th = vo.ansatz_from_state(e.state.numpy(), n)
            c = noisy((k, a, q, p, th))
            ref = vo.energy_dm(vo.run_circuit_dm(psi0, c[0], c[1], c[2], c[3], th, cls.NOISE_P1, cls.NOISE_P2), xs, zs, case["weights"])
            assert abs(e.energy - ref) < E_TOL, (t, b, e.energy, ref)
    with pytest.raises(ValueError):
        VecCircuitEnv(Noiseless, conf, dev, B, noise_channel="exact")
    with pytest.raises(ValueError):
        VecCircuitEnv(cls, conf, dev, B, noise_channel="channel")
