"""GPU: every entry point of the LDS-resident kernel family at EVERY compiled register size N = 1 ... 13 (LdsSizes of
csrc/vqe_api.hip) against the oracle - k_lds_state, k_lds_energy, the four k_lds_minimize<N, WIDE, NOISY>
instantiations (trace level), the environment step and the adjoint gradient.  The device L-BFGS at every size is
test_trajectory_parity of tests/test_lbfgs_gpu.py, whose table of cases (lbfgs_helpers.TRAJ_GATES) holds every N.  Each size has its own
workgroup geometry (Geo<N>: fewer amplitudes than lanes up to 5 qubits, one wave with 1 - 8 amplitudes per lane at
6 - 9, the unit path from 8, the register path from 10, 512 threads at 13), so no size stands in for another.

Inputs: tests/lds_cases.py (one seed per N; numpy oracle below 10 qubits, its C restatement from 10).  Tolerances are
the project's: 1e-12 on amplitudes, 1e-10 on energies, 1e-9 on trial points, 1e-10 x max(1, sum |c_k|) on gradients
(tests/test_grad_gpu.py).  At one qubit there are no CNOTs; everything else applies.  The circuit of a COBYLA case is the
first of its seeds whose walk hangs on no marginal decision (lds_cases.walk_is_decided: CPU only)."""
import numpy as np
import pytest

import lds_cases as lc
from helpers import random_gates, shift_grad, with_noise_gates

pytestmark = pytest.mark.gpu

SIZES = lc.SIZES
WIDE_SIZES = tuple(n for n in SIZES if n >= lc.WIDE_MIN)


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _gates(n, seed):
    rng = np.random.default_rng(seed)
    return random_gates(n, min(20 + 4 * n, 70), rng, p_cnot=0.4 if n > 1 else 0.0)


def _small_p(n):
    return min(3 * n, 10)


@pytest.mark.parametrize("n", SIZES)
def test_state(tq, n):
    """1. k_lds_state"""
    psi0, _ = lc.inputs(n)
    kind, q0, q1, pidx, th = _gates(n, 100 + n)
    eng = lc.engine(tq, n)
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    assert np.abs(eng.get_state(th) - lc.run_circuit(n, psi0, kind, q0, q1, pidx, th)).max() < lc.A_TOL
    eng.close()


@pytest.mark.parametrize("n", SIZES)
def test_energy_batch(tq, n):
    """2. k_lds_energy at perturbed angles; from 8 qubits part of the Hamiltonian is held as units"""
    psi0, ham = lc.inputs(n)
    kind, q0, q1, pidx, th = _gates(n, 200 + n)
    rng = np.random.default_rng(250 + n)
    ths = th + rng.normal(scale=0.3, size=(5, th.size))
    eng = lc.engine(tq, n)
    if n >= 8:
        assert eng.hamiltonian_layout()["units"] > 0
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    got = eng.energy_batch(ths)
    for b in range(ths.shape[0]):
        ref = lc.oracle_energy(n, psi0, (kind, q0, q1, pidx), ths[b], ham)
        assert abs(got[b] - ref) < lc.E_TOL, (n, b, got[b], ref)
    eng.close()


@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("n", SIZES)
def test_device_cobyla(tq, n, noisy):
    """3. / 4. k_lds_minimize<N, false, NOISY> on up to 64 parameters, every traced value and the walk"""
    gates, th = lc.cobyla_case(n, _small_p(n), 300 + n, noisy)
    eng = lc.engine(tq, n)
    lc.minimize_and_check(eng, tq, n, gates, th, noisy)
    eng.close()


def _pre_action(gates, P, ng, noisy):
    """The circuit the optimiser sees in an environment step whose new gate is gate ``ng`` (-1: none) - without it and,
    in a noisy circuit, without ITS channel -> (gates, the parameters that are variables, the hole or -1)"""
    kind, q0, q1, pidx = gates
    keep = np.ones(kind.size, bool)
    hole = -1
    if ng >= 0:
        keep[ng] = False
        if noisy:
            keep[ng + 1] = False
        if kind[ng] != 0:
            hole = int(pidx[ng])
    sel = [j for j in range(P) if j != hole]
    pp = np.where(pidx[keep] > hole, pidx[keep] - 1, pidx[keep]) if hole >= 0 else pidx[keep]
    return (kind[keep], q0[keep], q1[keep], pp), sel, hole


@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("n", SIZES)
def test_env_step_new_gate_in_the_middle(tq, n, noisy):
    """5. The environment step: COBYLA on the circuit without the new gate (noisy: nor its channel), float32 round trip,
    energy of the full circuit.  The new gate sits in the middle: a rotation (its parameter is a hole with variables
    on both sides), from two qubits on a CNOT as well, and a circuit without a new gate."""
    import c_oracle as co
    psi0, ham = lc.inputs(n)
    seed = 777000 + n
    maxfun = _small_p(n) + 1 + lc.AFTER_SIMPLEX + 8

    def build(b, j):
        """circuit b of the batch from its j-th seed -> ((gates as loaded, theta, new gate), the optimiser's problem)"""
        gates, th = lc.cobyla_circuit(n, _small_p(n), 410 + 10 * n + b + 100000 * j)
        th = th.astype(np.float32).astype(np.float64)
        kind = gates[0]
        if b == 0:
            rot = np.nonzero(kind != 0)[0]
            ng = int(rot[rot.size // 2])
            th[gates[3][ng]] = 0.0                    # a new rotation enters with theta = 0
        elif b == 1:
            ng = -1
        else:
            cn = np.nonzero(kind == 0)[0]
            ng = int(cn[cn.size // 2]) if cn.size else -1
        g = with_noise_gates(*gates) if noisy else gates
        ng = (2 * ng if noisy else ng) if ng >= 0 else -1
        pre, sel, _ = _pre_action(g, th.size, ng, noisy)
        return (g, th, ng), (n, pre, th[sel], maxfun, (seed, b, lc.P1, lc.P2) if noisy else None, None)

    cases = [lc.first_decided(lambda j, b=b: build(b, j), f"env-step n={n} circuit {b}{' noisy' if noisy else ''}")
             for b in range(3 if n > 1 else 2)]
    circuits = [(g, th) for g, th, _ in cases]
    new = [ng for _, _, ng in cases]
    eng = lc.engine(tq, n)
    x, xraw, f, nfev, traces = lc.traced_minimize(eng, tq, circuits, maxfun, (seed, 0, lc.P1, lc.P2) if noisy else None, new)
    off = 0
    for b, ((kind, q0, q1, pidx), th) in enumerate(circuits):
        P, ng = th.size, new[b]
        xb, xr = x[off:off + P], xraw[off:off + P]
        off += P
        pre, sel, hole = _pre_action((kind, q0, q1, pidx), P, ng, noisy)
        ft, xt = traces[b]
        lc.check_trace(tq, n, pre, th[sel], ft, xt[:, :len(sel)], int(nfev[b]), maxfun, (seed, b, lc.P1, lc.P2) if noisy else None)
        if hole >= 0:
            assert 0 < hole < P - 1 or P <= 2
            assert xb[hole] == th[hole] == 0.0
        assert np.array_equal(xb, xr.astype(np.float32).astype(np.float64))
        dr = co.noise_draws(seed, b, maxfun + 1, kind, lc.P1, lc.P2) if noisy else None
        e_full = lc.oracle_energy(n, psi0, (kind, q0, q1, pidx), xb, ham, dr)
        assert abs(f[b] - e_full) < lc.E_TOL, (n, b, f[b], e_full)
    eng.close()


@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("n", WIDE_SIZES)
def test_device_cobyla_wide(tq, n, noisy):
    """6. k_lds_minimize<N, true, NOISY>, just above 64 parameters (maxfun = P + 1 + 12): the rows context of the one-wave
    sizes, the workgroup-wide one from 10 qubits (with tiles at 12 and 13)."""
    P = 65
    gates, th = lc.cobyla_case(n, P, 500 + n, noisy)
    eng = lc.engine(tq, n)
    eng.batch_load([tq.Circuit(*gates, P)], [th])
    q = eng.batch_cobyla_placement(0)
    assert q["class"] == ("rows" if n <= 9 else "block") and q["pad"] == (8 if n in (10, 11) else 16), q
    lc.minimize_and_check(eng, tq, n, gates, th, noisy)
    eng.close()


@pytest.mark.parametrize("n", [n for n in WIDE_SIZES if n <= 9])
def test_small_circuit_in_a_wide_batch(tq, n):
    """6. One-wave sizes: next to a 70-parameter circuit a 40-parameter one runs the rows context on the global scratch
    (padding 16); alone it runs the plain variant (padding 8).  Its result is the same, bit for bit - and its walk is
    COBYLA's in both."""
    maxfun = 70 + 1 + lc.AFTER_SIMPLEX
    g40, t40 = lc.cobyla_case(n, 40, 600 + n, maxfun=maxfun)
    g70, t70 = lc.cobyla_case(n, 70, 650 + n, maxfun=maxfun)
    eng = lc.engine(tq, n)
    x1, _, f1, n1, tr1 = lc.traced_minimize(eng, tq, [(g40, t40)], maxfun)
    q_alone = eng.batch_cobyla_placement(0)
    x2, _, f2, n2, tr2 = lc.traced_minimize(eng, tq, [(g40, t40), (g70, t70)], maxfun)
    q_mixed = [eng.batch_cobyla_placement(b) for b in range(2)]
    assert (q_alone["class"], q_alone["pad"]) == ("global", 8), q_alone
    assert [(q["class"], q["pad"]) for q in q_mixed] == [("rows", 16), ("rows", 16)], q_mixed
    assert n1[0] == n2[0] and f1[0] == f2[0] and np.array_equal(x1, x2[:40])
    assert np.array_equal(tr1[0][0], tr2[0][0]) and np.array_equal(tr1[0][1], tr2[0][1])
    lc.check_trace(tq, n, g40, t40, tr2[0][0], tr2[0][1], int(n2[0]), maxfun)
    lc.check_trace(tq, n, g70, t70, tr2[1][0], tr2[1][1], int(n2[1]), maxfun)
    eng.close()


@pytest.mark.parametrize("n", SIZES)
def test_energy_grad(tq, n):
    """7. k_lds_energy_grad against the exact parameter shift on the oracle"""
    psi0, ham = lc.inputs(n)
    rng = np.random.default_rng(700 + n)
    kind, q0, q1, pidx, th = random_gates(n, min(12 + 3 * n, 40), rng, p_cnot=0.3 if n > 1 else 0.0)
    eng = lc.engine(tq, n)
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    e, g = eng.energy_grad(th)
    energy = lambda p0, k, a, b, p, t, h: lc.oracle_energy(n, p0, (k, a, b, p), t, h)
    g_ref = shift_grad(psi0, kind, q0, q1, pidx, th, ham, energy)
    scale = max(1.0, float(np.abs(ham[2]).sum()))
    assert np.abs(g - g_ref).max(initial=0.0) <= 1e-10 * scale, (n, np.abs(g - g_ref).max())
    assert abs(e - lc.oracle_energy(n, psi0, (kind, q0, q1, pidx), th, ham)) <= 1e-10 * scale
    eng.close()
