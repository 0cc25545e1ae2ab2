"""GPU: adjoint energy gradients on the streaming path (n >= 14; k_sg_lambda / k_sg_back / k_sg_reduce behind
vqe_set_stream_grad) against exact parameter shift on the CPU oracle, and a CircuitEnv with a gradient optim_alg at
14 qubits.  Tolerances are those of the LDS-path gradient tests: |g - g_ref|_inf <= 1e-10 max(1, sum |c|), the energy
to 1e-10 of the same scale.  The Hamiltonians are kept short where the oracle pays per term and per shifted angle."""
import numpy as np
import pytest

import su4_helpers as s4
import vqe_oracle as vo
from helpers import fermionic_hamiltonian, random_gates, random_hamiltonian, random_state

pytestmark = pytest.mark.gpu

K_SWEEP = 3      # kGradOpsPerSweep of csrc/vqe_stream_grad.h: the ops one backward sweep undoes


def _engine(n, ham, psi0, circ, stream_grad=True):
    import tensorrl_qas_amd as tq
    eng = tq.VQEEngine(n, 0)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    if circ is not None:
        eng.set_circuit(circ)
    if stream_grad:
        eng.set_stream_grad()
    return eng


def _circuit(kind, q0, q1, pidx, P):
    import tensorrl_qas_amd as tq
    return tq.Circuit(kind, q0, q1, pidx, P)


def _oracle_energy(psi0, kind, q0, q1, pidx, th, ham):
    return vo.energy_pauli(vo.run_circuit(psi0, kind, q0, q1, pidx, th), *ham)


def _shift_grad(psi0, kind, q0, q1, pidx, th, ham):
    """Exact parameter shift, gate by gate: dE/dtheta_j = sum over the gates g with parameter j of
    (E(theta_g + pi/2) - E(theta_g - pi/2)) / 2, each gate given its own copy of the angle."""
    grad = np.zeros(th.size)
    rot = [g for g in range(kind.size) if kind[g] in (1, 2, 3)]
    own = np.array([-1] * kind.size, np.int32)
    for i, g in enumerate(rot):
        own[g] = i
    base = np.array([th[pidx[g]] for g in rot])
    for i, g in enumerate(rot):
        tp, tm = base.copy(), base.copy()
        tp[i] += np.pi / 2
        tm[i] -= np.pi / 2
        d = 0.5 * (_oracle_energy(psi0, kind, q0, q1, own, tp, ham) - _oracle_energy(psi0, kind, q0, q1, own, tm, ham))
        grad[pidx[g]] += d
    return grad


def _scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


def _spread(ham, m, n, rng):
    """A Pauli sum on m qubits placed on m of n qubits (bit i -> bit sel[i]): the oracle pays per term, so the
    fermionic sums of the larger cases are built on fewer orbitals and spread over the register."""
    sel = np.sort(rng.choice(n, m, replace=False))
    move = lambda v: sum(((int(v) >> i) & 1) << int(sel[i]) for i in range(m))
    return (np.array([move(x) for x in ham[0]], np.uint64), np.array([move(z) for z in ham[1]], np.uint64), ham[2])


def _parity_gates(n, n_rot, rng):
    """random_gates (p_cnot = 0.3) cut or padded to n_rot rotations, three of them - RX, RY, RX on one qubit, no CNOT
    between - in a row: whatever the alignment of the K-op sweeps, two of the three share a sweep, and the second's
    partner mask then depends on the first's (the dependent-mask branch of the slot basis)."""
    kind, q0, q1, pidx, th = (list(v) for v in random_gates(n, 3 * n_rot, rng, p_cnot=0.3))
    out, rot = [], 0
    for k, a, b in zip(kind, q0, q1):
        if rot == n_rot - 3 and k != 0:
            break
        out.append((int(k), int(a), int(b)))
        rot += k != 0
    assert rot == n_rot - 3
    at = len(out) // 2
    q = int(rng.integers(n))
    out[at:at] = [(1, q, -1), (2, q, -1), (1, q, -1)]
    kind = np.array([g[0] for g in out], np.int32)
    pidx = np.full(kind.size, -1, np.int32)
    pidx[kind != 0] = np.arange(n_rot)
    theta = rng.uniform(-np.pi, np.pi, n_rot)
    return kind, np.array([g[1] for g in out], np.int32), np.array([g[2] for g in out], np.int32), pidx, theta


def test_default_is_the_refusal():
    import tensorrl_qas_amd as tq
    n = 14
    rng = np.random.default_rng(1)
    kind, q0, q1, pidx, th = random_gates(n, 10, rng, p_cnot=0.3)
    ham = random_hamiltonian(n, 6, rng)
    psi0 = random_state(n, rng)
    eng = _engine(n, ham, psi0, _circuit(kind, q0, q1, pidx, th.size), stream_grad=False)
    with pytest.raises(tq.VQEError):
        eng.energy_grad(th)
    assert abs(eng.energy(th) - _oracle_energy(psi0, kind, q0, q1, pidx, th, ham)) <= 1e-10 * _scale(ham)


@pytest.mark.parametrize("n", [14, 15, 16])
def test_grad_parity(n):
    rng = np.random.default_rng(303 + n)
    n_rot = {14: 13, 15: 11, 16: 7}[n]
    assert n_rot > K_SWEEP and n_rot % K_SWEEP and n_rot % 2      # a partial last sweep for K = 3 (and for K = 2)
    kind, q0, q1, pidx, th = _parity_gates(n, n_rot, rng)
    last_rot = int(np.nonzero(kind)[0].max())
    assert (kind[:last_rot] == 0).sum() >= 2      # CNOTs among the rotations: partner and sign masks of several bits
    psi0 = random_state(n, rng)
    m = {14: 14, 15: 10, 16: 8}[n]
    hams = [random_hamiltonian(n, {14: 34, 15: 20, 16: 10}[n], rng, real=False),
            _spread(fermionic_hamiltonian(m, n_hop=m, n_quad=m // 2, rng=rng, dressed=2), m, n, rng)]
    for ham in hams:
        eng = _engine(n, ham, psi0, _circuit(kind, q0, q1, pidx, th.size))
        assert not eng.device_info()["lds_path"]
        e, g = eng.energy_grad(th)
        g_ref = _shift_grad(psi0, kind, q0, q1, pidx, th, ham)
        scale = _scale(ham)
        print(n, "grad err", np.abs(g - g_ref).max(), "scale", scale)
        assert np.abs(g - g_ref).max() <= 1e-10 * scale, (n, np.abs(g - g_ref).max())
        assert abs(e - eng.energy(th)) <= 1e-10 * scale
        assert abs(e - _oracle_energy(psi0, kind, q0, q1, pidx, th, ham)) <= 1e-10 * scale


def test_two_qubit_rotations():
    n = 14
    rng = np.random.default_rng(70)
    g = s4.random_gates_su4(n, 16, rng)
    kind, q0, q1, pidx, th = g
    assert {s4.RXX, s4.RYY, s4.RZZ} <= set(kind.tolist())
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 20, rng, real=False)
    eng = _engine(n, ham, psi0, _circuit(kind, q0, q1, pidx, th.size))
    e, gr = eng.energy_grad(th)
    g_ref = s4.shift_grad(psi0, kind, q0, q1, pidx, th, ham)
    scale = _scale(ham)
    assert np.abs(gr - g_ref).max() <= 1e-10 * scale, np.abs(gr - g_ref).max()
    assert abs(e - s4.energy(psi0, kind, q0, q1, pidx, th, ham)) <= 1e-10 * scale
    assert abs(e - eng.energy(th)) <= 1e-10 * scale


def test_work_buffers_across_alternating_uses():
    """One handle, energy and gradient runs of different batch sizes in turn: the streaming work buffers grow, are used
    again by a smaller batch, and the block partials are sized by the energy run and by the gradient run in turn.
    Energy of one stream, energy and gradient of three, the energy of the three again (the gradient's backward sweep
    undid their states: the energy run makes them anew), energy of one.  Tolerances: those of test_two_qubit_rotations
    here and of test_streaming_path (tests/test_hip_parity.py) at n = 14."""
    n = 14
    rng = np.random.default_rng(1414)
    #       RY  RX  CNOT RXX     RZ  RY  RZZ     RX
    kind = np.array([2, 1, 0, s4.RXX, 3, 2, s4.RZZ, 1], np.int32)
    q0 = np.array([0, 13, 0, 5, 7, 9, 12, 3], np.int32)
    q1 = np.array([-1, -1, 7, 11, -1, -1, 2, -1], np.int32)
    pidx = np.array([0, 1, -1, 2, 3, 4, 5, 6], np.int32)
    P = 7
    xs, zs = [], []
    for x in (0, 0, 1 << 5 | 1 << 11, 1 << 5 | 1 << 11, 1 | 1 << 7 | 1 << 12, 1 | 1 << 7 | 1 << 12):      # two X masks besides the diagonal
        z = int(rng.integers(0, 1 << n))
        if bin(x & z).count("1") % 2:          # an even number of Y factors: every term Hermitian on its own
            z ^= x & -x
        xs.append(x); zs.append(z)
    ham = (np.array(xs, np.uint64), np.array(zs, np.uint64), rng.normal(size=len(xs)))
    assert len(set(xs) - {0}) >= 2
    psi0 = random_state(n, rng)
    eng = _engine(n, ham, psi0, _circuit(kind, q0, q1, pidx, P))
    assert not eng.device_info()["lds_path"]
    scale = _scale(ham)
    th1 = rng.uniform(-np.pi, np.pi, P)
    th3 = rng.uniform(-np.pi, np.pi, (3, P))
    e1_ref = s4.energy(psi0, kind, q0, q1, pidx, th1, ham)
    e3_ref = np.array([s4.energy(psi0, kind, q0, q1, pidx, t, ham) for t in th3])
    assert abs(eng.energy(th1) - e1_ref) <= 1e-10
    e, g = eng.energy_grad_batch(th3)
    for b in range(3):
        g_ref = s4.shift_grad(psi0, kind, q0, q1, pidx, th3[b], ham)
        print("stream", b, "grad err", np.abs(g[b] - g_ref).max(), "energy err", abs(e[b] - e3_ref[b]), "scale", scale)
        assert np.abs(g[b] - g_ref).max() <= 1e-10 * scale
    assert np.abs(e - e3_ref).max() <= 1e-10 * scale
    assert np.abs(eng.energy_batch(th3) - e3_ref).max() <= 1e-10
    assert abs(eng.energy(th1) - e1_ref) <= 1e-10


def test_untiled_forward_path():
    """More than 4096 terms: stream_tiled() is false, the forward pass is k_s_opk's.  The oracle pays for every term
    at every shifted angle, hence the short circuit."""
    n = 14
    rng = np.random.default_rng(4097)
    # RY q2, CNOT 2->9, RX q9, RZ q9, CNOT 9->0, RY q0, RX q5
    kind = np.array([2, 0, 1, 3, 0, 2, 1], np.int32)
    q0 = np.array([2, 2, 9, 9, 9, 0, 5], np.int32)
    q1 = np.array([-1, 9, -1, -1, 0, -1, -1], np.int32)
    pidx = np.array([0, -1, 1, 2, -1, 3, 4], np.int32)
    th = rng.uniform(-np.pi, np.pi, 5)
    assert th.size > K_SWEEP and th.size % K_SWEEP
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 4100, rng, real=False)
    eng = _engine(n, ham, psi0, _circuit(kind, q0, q1, pidx, th.size))
    assert eng.hamiltonian_terms()[0] > 4096
    e, g = eng.energy_grad(th)
    g_ref = _shift_grad(psi0, kind, q0, q1, pidx, th, ham)
    scale = _scale(ham)
    assert np.abs(g - g_ref).max() <= 1e-10 * scale, np.abs(g - g_ref).max()
    assert abs(e - _oracle_energy(psi0, kind, q0, q1, pidx, th, ham)) <= 1e-10 * scale
    assert abs(e - eng.energy(th)) <= 1e-10 * scale


def test_shared_and_unused_parameters():
    n = 14
    rng = np.random.default_rng(7)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 20, rng, real=False)
    # parameter 0 drives an RY on q1 and an RX on q11, parameter 2 drives no gate
    kind = np.array([2, 0, 1, 3, 0, 2], np.int32)
    q0 = np.array([1, 1, 11, 0, 11, 13], np.int32)
    q1 = np.array([-1, 2, -1, -1, 0, -1], np.int32)
    pidx = np.array([0, -1, 0, 1, -1, 3], np.int32)
    th = np.array([0.7, -1.1, 2.0, 0.4])
    eng = _engine(n, ham, psi0, _circuit(kind, q0, q1, pidx, 4))
    e, g = eng.energy_grad(th)
    g_ref = _shift_grad(psi0, kind, q0, q1, pidx, th, ham)
    assert g[2] == 0.0
    assert np.abs(g - g_ref).max() <= 1e-10 * _scale(ham)
    h = 1e-5
    tp, tm = th.copy(), th.copy()
    tp[0] += h
    tm[0] -= h
    fd = (_oracle_energy(psi0, kind, q0, q1, pidx, tp, ham) - _oracle_energy(psi0, kind, q0, q1, pidx, tm, ham)) / (2 * h)
    assert abs(g[0] - fd) < 1e-7


def test_batch_entry_points():
    import tensorrl_qas_amd as tq
    n = 14
    rng = np.random.default_rng(31)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, n_hop=n, n_quad=n // 2, rng=rng, dressed=1)
    raw = [random_gates(n, 17, rng, p_cnot=0.3),
           (np.zeros(3, np.int32), np.array([0, 5, 9], np.int32), np.array([1, 2, 13], np.int32),      # CNOTs only: no op
            np.full(3, -1, np.int32), np.zeros(0)),
           random_gates(n, 8, rng, p_cnot=0.3),
           (np.array([0, 2], np.int32), np.array([3, 4], np.int32), np.array([4, -1], np.int32),       # one rotation
            np.array([-1, 0], np.int32), np.array([0.9])),
           random_gates(n, 29, rng, p_cnot=0.3)]
    circs = [tq.Circuit(*g[:4], g[4].size) for g in raw]
    thetas = [g[4] for g in raw]
    assert len({int((c.kind != 0).sum()) for c in circs}) == 5
    eng = _engine(n, ham, psi0, None)
    eng.batch_load(circs, thetas)
    eng.batch_run_energy_grad()
    _, f, _ = eng.batch_fetch(want_x=False)
    gcat = eng.batch_fetch_grad()
    off = 0
    for c, th, fb in zip(circs, thetas, f):
        eng.set_circuit(c)
        e1, g1 = eng.energy_grad(th)
        assert abs(fb - e1) <= 1e-12
        assert np.abs(gcat[off:off + th.size] - g1).max(initial=0.0) <= 1e-12
        off += th.size
    assert off == gcat.size
    c = circs[-1]
    eng.set_circuit(c)
    ths = np.stack([thetas[-1] + 0.1 * k for k in range(5)])
    e, g = eng.energy_grad_batch(ths)
    assert g.shape == (5, c.n_params)
    assert np.abs(e - eng.energy_batch(ths)).max() <= 1e-10
    e0, g0 = eng.energy_grad(ths[3])
    assert abs(e[3] - e0) <= 1e-12 and np.abs(g[3] - g0).max() <= 1e-12


def test_term_shards_sum():
    n = 14
    rng = np.random.default_rng(5)
    kind, q0, q1, pidx, th = random_gates(n, 20, rng, p_cnot=0.3)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, n_hop=14, n_quad=8, rng=rng, dressed=2)
    circ = _circuit(kind, q0, q1, pidx, th.size)
    e, g = _engine(n, ham, psi0, circ).energy_grad(th)
    parts = []
    for r in range(2):
        eng = _engine(n, ham, psi0, circ)
        eng.set_term_shard(r, 2)
        parts.append(eng.energy_grad(th))
    scale = _scale(ham)
    assert abs(parts[0][0] + parts[1][0] - e) <= 1e-12 * scale
    assert np.abs(parts[0][1] + parts[1][1] - g).max() <= 1e-12 * scale


def test_handle_hygiene():
    n = 14
    rng = np.random.default_rng(11)
    kind, q0, q1, pidx, th = random_gates(n, 22, rng, p_cnot=0.3)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 24, rng, real=False)
    eng = _engine(n, ham, psi0, _circuit(kind, q0, q1, pidx, th.size))
    psi = vo.run_circuit(psi0, kind, q0, q1, pidx, th)
    e_ref = vo.energy_pauli(psi, *ham)
    scale = _scale(ham)
    e_a = eng.energy(th)
    e1, g1 = eng.energy_grad(th)
    e_b = eng.energy(th)
    state = eng.get_state(th)
    assert abs(e_a - e_ref) <= 1e-10 * scale and abs(e_b - e_ref) <= 1e-10 * scale
    assert np.abs(state - psi).max() <= 1e-12
    e2, g2 = eng.energy_grad(th)
    e3, g3 = eng.energy_grad(th)
    assert e2 == e3 and np.array_equal(g2, g3)
    assert abs(e1 - e2) <= 1e-12 and np.abs(g1 - g2).max() <= 1e-12
    # the same on a resident batch, whose plans outlive the runs: energy, gradient, energy
    eng.batch_load([_circuit(kind, q0, q1, pidx, th.size)], [th])
    eng.batch_run_energy()
    f0 = eng.batch_fetch(want_x=False)[1][0]
    eng.batch_run_energy_grad()
    f1 = eng.batch_fetch(want_x=False)[1][0]
    eng.batch_run_energy()
    f2 = eng.batch_fetch(want_x=False)[1][0]
    assert max(abs(f0 - e_ref), abs(f1 - e_ref), abs(f2 - e_ref)) <= 1e-10 * scale
    assert np.array_equal(eng.batch_fetch_grad(), g2)


def test_refusals_with_the_setting_on():
    import tensorrl_qas_amd as tq
    n = 14
    rng = np.random.default_rng(9)
    kind, q0, q1, pidx, th = random_gates(n, 14, rng, p_cnot=0.3)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 12, rng)
    circ = _circuit(kind, q0, q1, pidx, th.size)
    e_ref = _oracle_energy(psi0, kind, q0, q1, pidx, th, ham)
    eng = _engine(n, ham, psi0, circ)
    e0, g0 = eng.energy_grad(th)

    def refused(setup, undo):
        with pytest.raises(tq.VQEError):      # (the exact channel mode is refused by its setter at n >= 14)
            setup(eng)
            eng.energy_grad(th)
        undo(eng)
        assert abs(eng.energy(th) - e_ref) <= 1e-10 * _scale(ham)
        e, g = eng.energy_grad(th)
        assert abs(e - e0) <= 1e-12 and np.abs(g - g0).max() <= 1e-12

    refused(lambda e: e.set_noise(0.01, 0.0, 1), lambda e: e.set_noise(0.0, 0.0, 1))
    refused(lambda e: e.set_noise_mode(1), lambda e: e.set_noise_mode(0))
    refused(lambda e: e.set_shot_noise(0.1, 3), lambda e: e.set_shot_noise(0.0, 3))
    refused(lambda e: e.set_amplitude_shard(0, 2), lambda e: e.set_amplitude_shard(0, 1))
    with pytest.raises(tq.VQEError):
        eng.minimize_lbfgs(th, maxfun=5)
    assert abs(eng.energy(th) - e_ref) <= 1e-10 * _scale(ham)
    # switched off again: the refusal of the default
    eng.set_stream_grad(False)
    with pytest.raises(tq.VQEError):
        eng.energy_grad(th)


def test_circuit_env_lbfgsb_at_14_qubits(tmp_path):
    """A 14-qubit Heisenberg chain (built as tests/test_configs_gpu.py builds its 20-qubit one, with the synthetic init
    circuit) and optim_alg = L-BFGS-B: the environment switches the streaming gradient on for its engine."""
    import torch
    from tensorrl_qas_amd import synthetic
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    n = 14
    bound = float(3 * (n - 1) + n)
    conf = synthetic.write_chain_dataset(str(tmp_path / "dmrg-to-qc"), n, eigvals=[-bound, bound])
    conf["non_local_opt"]["global_iters"] = 5
    conf["non_local_opt"]["optim_alg"] = "L-BFGS-B"
    env = CircuitEnv(conf, torch.device("cuda:0"))
    assert env.optimizer_kind == "host_gradient" and not env.engine.device_info()["lds_path"]
    ham = (env.ham.xmask, env.ham.zmask, env.ham.coeff)
    scale = _scale(ham)
    psi0 = vo.statevector_from_qasm(open(env.spec.init_circuit_path()).read())
    env.reset()
    table = env._actions_table
    nq = n * (n - 1)

    def state_energy(state):
        k, a, b, p, th = vo.ansatz_from_state(state.numpy(), n)
        return vo.energy_pauli(vo.run_circuit(psi0, k, a, b, p, th), *ham)

    for ai in (nq + 3 * 3 + 1, 5 * (n - 1) + 0, nq + 5 * 3 + 0):      # RY q3, CNOT 5->6, RX q5
        prev = env.state.clone()
        env.step(table[ai])
        assert env.nfev >= 1
        assert abs(env.energy - state_energy(env.state)) <= 1e-10 * scale
        before = env.state.clone()                    # the full circuit at the angles the step started from
        rot = prev[:, n:n + 3] == 1
        before[:, n + 3:][rot] = prev[:, n + 3:][rot]
        assert env.energy <= state_energy(before) + 1e-10
