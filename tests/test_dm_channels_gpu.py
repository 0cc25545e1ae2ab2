"""GPU: Kraus channels in the noise slots of the exact channel mode (vqe_set_noise_kraus) and RXX / RYY / RZZ as block
members (vqe_set_dm_rot2), DESIGN 4.16 - serial path, batched path, adjoint gradient, device COBYLA and L-BFGS, the
environment batch.

Reference: tests/dm_kraus_oracle.py, explicit Kraus sums and 2^n x 2^n gate matrices on a dense rho (tied to the
project's oracle channel by tests/test_dm_channels_cpu.py), and its exact shift gradient - exact because a channel is
linear and every tested parameter belongs to one gate.  Tolerance: TOL = 1e-10 max(1, sum |c_k|), as
tests/test_dm_grad_gpu.py defines it, on every energy and every gradient component.  Closed forms where there are any."""
import functools

import numpy as np
import pytest

import dm_kraus_oracle as ko
import vqe_oracle as vo
from helpers import random_hamiltonian, random_state

pytestmark = pytest.mark.gpu
TOL = 1e-10
ESTATE, EINVAL = -1, -22
P1, P2 = 0.03, 0.07      # the depolarising channels of a slot without an override


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


def _engine(tq, n, psi0, ham, K1=None, K2=None, batched=-1, grad=True, rot2=False, p=(P1, P2), mode=1):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(p[0], p[1], 11)
    eng.set_noise_mode(mode)
    eng.set_dm_batched(batched)
    eng.set_dm_grad(grad)
    eng.set_dm_rot2(rot2)
    if K1 is not None or K2 is not None:
        eng.set_noise_kraus(K1, K2)
    return eng


def _circ(tq, c):
    return tq.Circuit(c[0], c[1], c[2], c[3], c[4].size)


def _zero_state(n):
    v = np.zeros(1 << n, np.complex128)
    v[0] = 1.0
    return v


def _gates(gates):
    """(kind, q0, q1, theta or None) per gate -> the five arrays"""
    kind, q0, q1, pidx, th = [], [], [], [], []
    for k, a, b, t in gates:
        kind.append(k), q0.append(a), q1.append(b)
        if t is None:
            pidx.append(-1)
        else:
            pidx.append(len(th)), th.append(float(t))
    return (np.array(kind, np.int32), np.array(q0, np.int32), np.array(q1, np.int32), np.array(pidx, np.int32), np.array(th, np.float64))


def _random_circuit(n, G, rng, rot2=False):
    """G gates, a channel behind every one: DEPOL1 behind a rotation, DEPOL2 behind a CNOT or a two-qubit rotation - in
    either order of the gate's qubits, so that both orientations of the two-qubit table are met."""
    gates = []
    for _ in range(G):
        a = int(rng.integers(n))
        b = int((a + 1 + rng.integers(n - 1)) % n)
        pick = rng.random()
        if pick < 0.4:
            gates.append((1 + int(rng.integers(3)), a, -1, rng.uniform(-np.pi, np.pi)))
            gates.append((4, a, -1, None))
            continue
        if rot2 and pick < 0.75:
            gates.append((6 + int(rng.integers(3)), a, b, rng.uniform(-np.pi, np.pi)))
        else:
            gates.append((0, a, b, None))
        gates.append((5, b, a, None) if rng.random() < 0.5 else (5, a, b, None))
    return _gates(gates)


def _kraus(K1, K2, p=(P1, P2)):
    """the Kraus sets the helper applies: an empty slot runs the depolarising channel of set_noise"""
    return (ko.depol1(p[0]) if K1 is None else K1), (ko.depol2(p[1]) if K2 is None else K2)


def _ref(psi0, ham, c, theta, K1, K2, p=(P1, P2), grad=True):
    k1, k2 = _kraus(K1, K2, p)
    e = ko.circuit_energy(psi0, c[0], c[1], c[2], c[3], theta, k1, k2, ham)
    return e, (ko.shift_grad(psi0, c[0], c[1], c[2], c[3], theta, k1, k2, ham) if grad else None)


def _energies(tq, eng, circuits, thetas=None):
    eng.batch_load([_circ(tq, c) for c in circuits], [c[4] for c in circuits] if thetas is None else thetas)
    eng.batch_run_energy()
    return eng.batch_fetch(want_x=False)[1].copy()


def _grads(tq, eng, circuits):
    eng.batch_load([_circ(tq, c) for c in circuits], [c[4] for c in circuits])
    eng.batch_run_energy_grad()
    f = eng.batch_fetch(want_x=False)[1].copy()
    g = eng.batch_fetch_grad()
    off = np.concatenate([[0], np.cumsum([c[4].size for c in circuits])])
    return f, [g[off[b]:off[b + 1]].copy() for b in range(len(circuits))]


def _check_against(tq, n, psi0, ham, circuits, ref, K1, K2, rot2=False, p=(P1, P2)):
    """serial energies, batched energies and the gradients of the batch against ref = [(E, grad)]"""
    scale = _scale(ham)
    serial = _engine(tq, n, psi0, ham, K1, K2, batched=0, grad=False, rot2=rot2, p=p)
    batched = _engine(tq, n, psi0, ham, K1, K2, rot2=rot2, p=p)
    es = _energies(tq, serial, circuits)
    eb = _energies(tq, batched, circuits)
    f, g = _grads(tq, batched, circuits)
    assert np.array_equal(f, eb)                                  # the gradient run's E is the energy run's
    for b, (e_ref, g_ref) in enumerate(ref):
        dg = np.abs(g[b] - g_ref).max(initial=0.0)
        print(f"n={n} circuit {b}: serial |dE|={abs(es[b] - e_ref):.2e} batched |dE|={abs(eb[b] - e_ref):.2e} |dg|={dg:.2e} "
              f"max|g|={np.abs(g_ref).max(initial=0.0):.2e}")
        assert abs(es[b] - e_ref) <= TOL * scale, (b, es[b], e_ref)
        assert abs(eb[b] - e_ref) <= TOL * scale, (b, eb[b], e_ref)
        assert dg <= TOL * scale, (b, dg)
    return serial, batched


# ---- 1. closed forms ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3])
def test_closed_forms_from_the_zero_state(tq, n):
    ch = tq.channels
    psi0 = _zero_state(n)
    q = n - 1
    z_q = (np.array([0], np.uint64), np.array([1 << q], np.uint64), np.array([1.0]))
    x_q = (np.array([1 << q], np.uint64), np.array([0], np.uint64), np.array([1.0]))
    for batched in (0, -1):
        # RX(pi) then amplitude damping: |1> falls to |0> with probability gamma
        for gamma in (0.0, 0.3, 1.0):
            eng = _engine(tq, n, psi0, z_q, ch.amplitude_damping(gamma), None, batched=batched, grad=False)
            e = _energies(tq, eng, [_gates([(1, q, -1, np.pi), (4, q, -1, None)])])[0]
            assert abs(e - (2.0 * gamma - 1.0)) <= TOL, (batched, gamma, e)
        # full dephasing behind RY(pi/2) removes the coherence <X> measures
        for K1, want in ((ch.dephasing(0.5), 0.0), (ch.dephasing(0.0), None)):
            eng = _engine(tq, n, psi0, x_q, K1, None, batched=batched, grad=False)
            e = _energies(tq, eng, [_gates([(2, q, -1, np.pi / 2), (4, q, -1, None)])])[0]
            if want is None:
                assert abs(abs(e) - 1.0) <= TOL, e       # without the channel the state is an X eigenstate
            else:
                assert abs(e - want) <= TOL, (batched, e)
        # gamma = 1 behind every gate: every touched qubit is reset, the state stays |0...0>
        rng = np.random.default_rng(6100 + n)
        ham = random_hamiltonian(n, 12, rng, real=False)
        ham[0][:4] = 0                                             # some diagonal terms for sure
        c = _random_circuit(n, 10, rng)
        one = ch.amplitude_damping(1.0)
        eng = _engine(tq, n, psi0, ham, one, ch.tensor(one, one), batched=batched, grad=False)
        e = _energies(tq, eng, [c])[0]
        want = float(np.real(ko.hamiltonian(n, *ham)[0, 0]))
        assert abs(want) > 1e-3 and abs(e - want) <= TOL * _scale(ham), (batched, e, want)


# ---- 2. orientation of the two-qubit slot -----------------------------------------------------------------------------------

def test_only_the_gates_q0_is_damped(tq):
    """K2 = amplitude damping (x) identity through DEPOL2(q0=2, q1=0) and DEPOL2(q0=0, q1=2) behind X rotations on both
    qubits: <Z> of the gate's q0 is 1 - 2 (1 - gamma) sin^2(theta/2), <Z> of its q1 stays cos(theta).  With the
    depolarising channel's orientation (pos = 0 whatever the order) one of the spellings damps the wrong qubit."""
    ch = tq.channels
    n, gamma, t0, t2 = 3, 0.6, 1.1, 2.3
    psi0 = _zero_state(n)
    ham = (np.array([0, 0], np.uint64), np.array([1, 4], np.uint64), np.array([1.0, -0.37]))      # Z_0 - 0.37 Z_2
    K2 = ch.tensor(ch.amplitude_damping(gamma), ch.identity(2))
    damped = lambda t: 1.0 - 2.0 * (1.0 - gamma) * np.sin(t / 2) ** 2
    for first in (0, 2):                                          # which rotation opens the window: a = 0 or a = 2
        rots = [(1, 0, -1, t0), (1, 2, -1, t2)] if first == 0 else [(1, 2, -1, t2), (1, 0, -1, t0)]
        for d0, d1 in ((2, 0), (0, 2)):
            c = _gates(rots + [(5, d0, d1, None)])
            want = (damped(t0) if d0 == 0 else np.cos(t0)) - 0.37 * (damped(t2) if d0 == 2 else np.cos(t2))
            wrong = (damped(t0) if d0 == 2 else np.cos(t0)) - 0.37 * (damped(t2) if d0 == 0 else np.cos(t2))
            assert abs(want - wrong) > 0.1
            for batched in (0, -1):
                eng = _engine(tq, n, psi0, ham, None, K2, batched=batched, grad=False)
                e = _energies(tq, eng, [c])[0]
                assert abs(e - want) <= TOL * _scale(ham), (first, d0, d1, batched, e, want, wrong)
            assert abs(_ref(psi0, ham, c, c[4], None, K2, grad=False)[0] - want) <= 1e-13      # the helper agrees


# ---- 3. parity with the helper --------------------------------------------------------------------------------------------

def _combo(tq, name):
    ch = tq.channels
    return {"damping+depol2": (ch.amplitude_damping(0.15), ch.two_qubit_depolarizing(0.08)),
            "dephasing+product": (ch.dephasing(0.1), ch.tensor(ch.amplitude_damping(0.3), ch.bit_flip(0.2))),
            "only-K1": (ch.independent_xz(0.12), None),
            "only-K2": (None, ch.tensor(ch.amplitude_damping(0.25), ch.dephasing(0.1)))}[name]


@functools.lru_cache(maxsize=None)
def _parity_case(n, rot2):
    """A batch of three circuits of 6, 10 and 14 gates with a channel behind every gate; made once, shared, never modified"""
    rng = np.random.default_rng(6200 + 10 * n + int(rot2))
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 6 + 3 * n, rng, real=False)
    return psi0, ham, [_random_circuit(n, G, rng, rot2=rot2) for G in (6, 10, 14)]


@functools.lru_cache(maxsize=None)
def _parity_ref(n, rot2, name):
    import tensorrl_qas_amd as t
    psi0, ham, circuits = _parity_case(n, rot2)
    K1, K2 = (None, None) if name == "depolarising" else _combo(t, name)
    return [_ref(psi0, ham, c, c[4], K1, K2) for c in circuits]


@pytest.mark.parametrize("name", ["damping+depol2", "dephasing+product", "only-K1", "only-K2"])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_parity_with_the_dense_helper(tq, n, name):
    psi0, ham, circuits = _parity_case(n, False)
    assert [len(c[0]) for c in circuits] == [12, 20, 28]
    assert any(np.any((c[0] == 5) & (c[1] > c[2])) for c in circuits) and any(np.any((c[0] == 5) & (c[1] < c[2])) for c in circuits)
    K1, K2 = _combo(tq, name)
    ref = _parity_ref(n, False, name)
    assert max(np.abs(g).max() for _, g in ref) > 1e-3
    _, batched = _check_against(tq, n, psi0, ham, circuits, ref, K1, K2)
    assert batched.noise_kraus_info() == {"n1": 0 if K1 is None else len(K1), "n2": 0 if K2 is None else len(K2)}
    # a circuit alone and chunks of one: what the batch gave, bit for bit
    f, g = _grads(tq, batched, circuits)
    f1, g1 = _grads(tq, batched, circuits[1:2])
    assert f1[0] == f[1] and np.array_equal(g1[0], g[1])
    batched.set_dm_batched(1)
    assert np.array_equal(_energies(tq, batched, circuits), f)


# ---- 4. the depolarising sets as an override ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 5])
def test_depolarising_kraus_sets_reproduce_the_built_in_channel(tq, n):
    ch = tq.channels
    psi0, ham, circuits = _parity_case(n, False)
    scale = _scale(ham)
    ref = _parity_ref(n, False, "depolarising")
    plain = _engine(tq, n, psi0, ham)
    over = _engine(tq, n, psi0, ham, ch.depolarizing(P1), ch.two_qubit_depolarizing(P2), p=(0.5, 0.5))      # p1 / p2 play no part
    fp, gp = _grads(tq, plain, circuits)
    fo, go = _grads(tq, over, circuits)
    for b in range(len(circuits)):
        print(f"n={n} circuit {b}: |E_override - E_builtin|={abs(fo[b] - fp[b]):.2e} |dg|={np.abs(go[b] - gp[b]).max():.2e}")
        assert abs(fo[b] - fp[b]) <= TOL * scale and np.abs(go[b] - gp[b]).max() <= TOL * scale
        assert abs(fp[b] - ref[b][0]) <= TOL * scale and np.abs(gp[b] - ref[b][1]).max() <= TOL * scale
    for e in (plain, over):
        e.set_dm_batched(0)
    es = _energies(tq, over, circuits)
    assert np.abs(es - _energies(tq, plain, circuits)).max() <= TOL * scale


# ---- 5. SU(4): two-qubit rotations in the exact channel mode ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["depolarising", "dephasing+product"])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_two_qubit_rotations_against_the_helper(tq, n, name):
    psi0, ham, circuits = _parity_case(n, True)
    kinds = np.concatenate([c[0] for c in circuits])
    assert all(np.any(kinds == k) for k in (0, 4, 5, 6, 7, 8)) and np.any((kinds >= 1) & (kinds <= 3))
    K1, K2 = (None, None) if name == "depolarising" else _combo(tq, name)
    ref = _parity_ref(n, True, name)
    assert max(np.abs(g).max() for _, g in ref) > 1e-3
    _check_against(tq, n, psi0, ham, circuits, ref, K1, K2, rot2=True)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_noiseless_two_qubit_rotations_equal_the_state_vector(tq, n):
    """p1 = p2 = 0, no override: the channels are identities, so mode 1 with rot2 is the state-vector engine's energy
    and gradient (mode 0 takes RXX / RYY / RZZ on its own kernels)."""
    psi0, ham, circuits = _parity_case(n, True)
    scale = _scale(ham)
    dm = _engine(tq, n, psi0, ham, rot2=True, p=(0.0, 0.0))
    sv = _engine(tq, n, psi0, ham, p=(0.0, 0.0), mode=0, batched=0, grad=False)
    f, g = _grads(tq, dm, circuits)
    dm.set_dm_batched(0)
    fs = _energies(tq, dm, circuits)
    for b, c in enumerate(circuits):
        keep = (c[0] != 4) & (c[0] != 5)                          # mode 0 gets the gates without the (identity) channels
        sv.set_circuit(_circ(tq, tuple(v[keep] for v in c[:4]) + (c[4],)))
        e0, g0 = sv.energy_grad(c[4])
        print(f"n={n} circuit {b}: |dE|={abs(f[b] - e0):.2e} serial |dE|={abs(fs[b] - e0):.2e} |dg|={np.abs(g[b] - g0).max():.2e}")
        assert abs(f[b] - e0) <= TOL * scale and abs(fs[b] - e0) <= TOL * scale and np.abs(g[b] - g0).max() <= TOL * scale


@pytest.mark.parametrize("optimiser", ["cobyla", "lbfgs"])
def test_device_optimisers_on_a_batch_with_two_qubit_rotations(tq, optimiser):
    n = 3
    psi0, ham, circuits = _parity_case(n, True)
    scale = _scale(ham)
    K1, K2 = _combo(tq, "dephasing+product")
    eng = _engine(tq, n, psi0, ham, K1, K2, rot2=True)
    f0 = _energies(tq, eng, circuits)
    if optimiser == "cobyla":
        eng.batch_run_minimize(1.0, 1e-4, 60)
    else:
        eng.batch_run_minimize_lbfgs(history=3, maxiter=6, maxfun=60)
    x, f, nfev = eng.batch_fetch()
    off = 0
    for b, c in enumerate(circuits):
        P = c[4].size
        e = _ref(psi0, ham, c, x[off:off + P], K1, K2, grad=False)[0]
        print(f"{optimiser} circuit {b}: nfev={nfev[b]} f0={f0[b]:.8f} f={f[b]:.8f} |f - E(x)|={abs(f[b] - e):.2e}")
        assert f[b] <= f0[b], (b, f[b], f0[b])
        assert abs(f[b] - e) <= TOL * scale, (b, f[b], e)
        off += P
    assert np.any(f < f0 - 1e-3) and nfev.max() > 3


# ---- 6. switches and refusals -----------------------------------------------------------------------------------------------

def test_rot2_switch_and_refusals(tq):
    ch = tq.channels
    n = 3
    psi0, ham, circuits = _parity_case(n, True)
    plain = _parity_case(n, False)[2]
    c, th = circuits[0], circuits[0][4]
    # rot2 off: the refusals of today, code and text
    eng = _engine(tq, n, psi0, ham)
    eng.batch_load([_circ(tq, c)], [th])
    for run in (eng.batch_run_energy, lambda: eng.batch_run_minimize(1.0, 1e-4, 20), eng.batch_run_energy_grad):
        with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:.*does not take RXX / RYY / RZZ gates \(use Pauli-trajectory noise"):
            run()
    eng.set_circuit(_circ(tq, c))
    with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:.*RXX"):
        eng.energy_grad(th)
    eng.set_dm_rot2(True)
    on = eng.energy(th)
    eng.set_dm_rot2(False)
    with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:.*RXX"):
        eng.energy(th)
    assert abs(on - _ref(psi0, ham, c, th, None, None, grad=False)[0]) <= TOL * _scale(ham)
    tq.VQEEngine(14).set_dm_rot2(True)                            # accepted on any handle

    # validation: VQE_EINVAL, the installed sets stay
    K1, K2 = _combo(tq, "dephasing+product")
    eng = _engine(tq, n, psi0, ham, K1, K2)
    info = eng.noise_kraus_info()
    assert info == {"n1": 2, "n2": 4}
    before = _energies(tq, eng, plain)
    bad = [(0.9 * K1, None), (None, K2[:3]), (np.zeros((17, 2, 2)), None), (None, np.zeros((65, 4, 4))),
           (K1 * np.array([1.0, 1.0 + 1e-11])[:, None, None], None), (np.full((1, 2, 2), np.nan), None)]
    for b1, b2 in bad:
        with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:"):
            eng.set_noise_kraus(b1, b2)
        assert eng.noise_kraus_info() == info
    assert np.array_equal(_energies(tq, eng, plain), before)
    eng.set_noise_kraus(np.concatenate([K1, np.zeros((14, 2, 2))]), np.concatenate([K2, np.zeros((60, 4, 4))]))      # the limits
    assert eng.noise_kraus_info() == {"n1": 16, "n2": 64}
    assert np.abs(_energies(tq, eng, plain) - before).max() <= TOL * _scale(ham)
    eng.set_noise_kraus(K1, K2)
    before = _energies(tq, eng, plain)

    # an override has no trajectory form: mode 0 runs and get_state are refused, nothing launched, counter unchanged
    cp = plain[0]
    eng.set_circuit(_circ(tq, cp))
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*Kraus"):
        eng.get_state(cp[4])                                      # in mode 1 too
    eng.set_noise_mode(0)
    calls = (eng.batch_run_energy, lambda: eng.batch_run_minimize(1.0, 1e-4, 20), lambda: eng.batch_run_env_step(1.0, 1e-4, 20),
             eng.batch_run_energy_grad, lambda: eng.batch_run_minimize_lbfgs(maxiter=1), lambda: eng.energy(cp[4]),
             lambda: eng.minimize_cobyla(cp[4], maxfun=20), lambda: eng.energy_grad(cp[4]), lambda: eng.get_state(cp[4]))
    for call in calls:
        with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*Kraus"):
            call()
    assert np.array_equal(eng.batch_fetch(want_x=False)[1], before)
    eng.set_noise_kraus(None, None)                               # removed: mode 0 runs again, at the counter of a new handle
    assert eng.noise_kraus_info() == {"n1": 0, "n2": 0}
    fresh = _engine(tq, n, psi0, ham, mode=0, batched=0, grad=False)
    fresh.set_circuit(_circ(tq, cp))
    assert eng.energy(cp[4]) == fresh.energy(cp[4]) and eng.energy(cp[4]) == fresh.energy(cp[4])
    assert np.array_equal(eng.get_state(cp[4]), fresh.get_state(cp[4]))


def test_one_handle_through_install_replace_remove(tq):
    """install -> replace -> one slot -> remove -> set_noise: at every step the bits of a fresh handle with the step's
    settings, on the serial path, the batched path and for the gradient - a table cached by (p1, p2) alone would not."""
    ch = tq.channels
    n = 3
    psi0, ham, circuits = _parity_case(n, False)
    a = _combo(tq, "dephasing+product")
    b = _combo(tq, "damping+depol2")
    steps = [dict(K=(None, None), p=(P1, P2)), dict(K=a, p=(P1, P2)), dict(K=b, p=(P1, P2)), dict(K=(b[0], None), p=(P1, P2)),
             dict(K=(None, a[1]), p=(P1, P2)), dict(K=(None, a[1]), p=(0.2, 0.3)), dict(K=(None, None), p=(0.2, 0.3)),
             dict(K=a, p=(0.2, 0.3)), dict(K=(None, None), p=(P1, P2))]
    one = _engine(tq, n, psi0, ham)
    seen = []
    for s in steps:
        one.set_noise(*s["p"], 11)                                # (a later set_noise does not remove the override)
        one.set_noise_kraus(*s["K"])
        fresh = _engine(tq, n, psi0, ham, s["K"][0], s["K"][1], p=s["p"])
        out = []
        for e in (one, fresh):
            e.set_dm_batched(-1)
            f, g = _grads(tq, e, circuits)
            e.set_dm_batched(0)
            out.append((f, np.concatenate(g), _energies(tq, e, circuits)))
        for x, y in zip(*out):
            assert np.array_equal(x, y), s
        seen.append(out[0][0])
    assert np.array_equal(seen[0], seen[-1]) and all(np.abs(seen[i] - seen[i + 1]).max() > 1e-6 for i in range(len(seen) - 1))


# ---- 7. environments ------------------------------------------------------------------------------------------------------

def test_vec_env_with_kraus_channels(tmp_path_factory):
    """VecCircuitEnv(noisy class, noise_channel="exact", noise_kraus=(K1, K2)): both host loops agree, and every reported
    energy is the helper's energy of that environment's circuit AT ITS REPORTED ANGLES (not another run's trajectory)."""
    import torch
    from helpers import load_case, make_data_root, oracle_init_state, reference_config
    from tensorrl_qas_amd import channels as ch
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv as cls
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    data_root = make_data_root(str(tmp_path_factory.mktemp("dmrg-to-qc")))
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2_noise", data_root)
    conf["non_local_opt"]["global_iters"] = 30
    dev = torch.device("cuda:0")
    B = 2
    K = (ch.amplitude_damping(0.02), ch.tensor(ch.amplitude_damping(0.05), ch.dephasing(0.03)))
    with pytest.raises(ValueError, match="noise_kraus"):
        VecCircuitEnv(cls, conf, dev, B, seed=4, noise_kraus=K)
    with pytest.raises(ValueError, match="noise_kraus"):
        VecCircuitEnv(cls, conf, dev, B, seed=4, noise_channel="trajectory", noise_kraus=K)
    vn = VecCircuitEnv(cls, conf, dev, B, seed=4, native=True, noise_channel="exact", noise_kraus=K)
    vp = VecCircuitEnv(cls, conf, dev, B, seed=4, native=False, noise_channel="exact", noise_kraus=K)
    assert vn.native and not vp.native and vp.engine.noise_kraus_info() == {"n1": 2, "n2": 4}
    assert torch.equal(vn.reset(), vp.reset())
    case = load_case("H2O_8q")
    n = vp.num_qubits
    psi0 = oracle_init_state(case)
    xs, zs = vo.pauli_masks(case["paulis"], n, reverse=False)
    ham = (xs, zs, case["weights"])
    table = vp.envs[0]._actions_table
    script = [[0, 56 + 1 * 3 + 1], [56 + 0 * 3 + 0, 1]]
    for t in range(2):
        acts = [table[script[b][t]] for b in range(B)]
        on, rn, dn = vn.step(acts)
        op, rp, dp = vp.step(acts)
        assert torch.equal(on, op) and torch.equal(rn, rp) and dn == dp, t
        for b in range(B):
            e, w = vp.envs[b], vn.envs[b]
            assert (w.energy, w.nfev) == (e.energy, e.nfev) and 1 <= e.nfev <= 30
            c = vo.ansatz_from_state(e.state.numpy(), n, noise=True)
            ref = ko.circuit_energy(psi0, c[0], c[1], c[2], c[3], c[4], K[0], K[1], ham)
            dep = vo.energy_dm(vo.run_circuit_dm(psi0, c[0], c[1], c[2], c[3], c[4], cls.NOISE_P1, cls.NOISE_P2), *ham)
            print(f"step {t} env {b}: nfev={e.nfev} E={e.energy:.10f} |dE|={abs(e.energy - ref):.2e} (depolarising: {dep:.10f})")
            assert abs(e.energy - ref) < 1e-10, (t, b, e.energy, ref)
            assert abs(dep - ref) > 1e-6                          # the override is what ran
