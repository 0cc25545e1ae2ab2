"""GPU: adjoint gradient and device L-BFGS on frozen Pauli-noise realisations (vqe_set_noise_grad).

Reference: tests/noise_grad_cases.py - the draws and the energy of tests/noise_pauli_oracle.py, the gradient of one
realisation by the exact parameter shift with the realisation's codes held fixed, E_T and its gradient summed in
ascending t.  Tolerance: the project's gradient tolerance, |g - g_ref|_inf and |E - E_ref| <= 1e-10 max(1, sum |c_k|).
The preconditions on the draws (tests/test_noise_grad_cpu.py checks them without a device) are asserted again in front
of every comparison that relies on them."""
import numpy as np
import pytest

import noise_grad_cases as ngc
import noise_pauli_oracle as npo
from helpers import random_gates, random_hamiltonian, random_state, with_noise_gates
from lbfgs_helpers import shared_unused_case

pytestmark = pytest.mark.gpu
TOL = 1e-10
ESTATE, EINVAL = -1, -22
P = (ngc.P1, ngc.P2)


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _engine(tq, n, psi0, ham, seed, T, hold=False, p=P, tables=(None, None)):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(p[0], p[1], seed)
    if tables[0] is not None or tables[1] is not None:
        eng.set_noise_pauli(*tables)
    eng.set_noise_grad(T, hold)
    return eng


def _load(tq, eng, circuits):
    eng.batch_load([tq.Circuit(*g, th.size) for g, th in circuits], [th for _, th in circuits])


def _offsets(circuits):
    return np.concatenate([[0], np.cumsum([th.size for _, th in circuits])])


def _grad_run(eng):
    eng.batch_run_energy_grad()
    return eng.batch_fetch(want_x=False)[1], eng.batch_fetch_grad()


# ---- 1. parity with the oracle ------------------------------------------------------------------------------------------------

def test_the_draws_of_the_parity_cases():
    assert ngc.parity_features() == {"none", "x_before_control", "y", "both"}


@pytest.mark.parametrize("n", ngc.PARITY_N)
def test_parity_with_the_oracle(tq, n):
    """n = 3: fewer amplitudes than a wave has lanes; 9: the last size before the N >= 10 branch of the patch, all nine
    gate kinds; 10: the first size after it; 13: lambda in global memory, a persistent grid smaller than the batch.
    70 gates + 70 noise gates: the patch walks three chunks of 64 gates.  T = 3, p1 = 0.2, p2 = 0.3."""
    assert ngc.parity_features() == {"none", "x_before_control", "y", "both"}      # (from the draws alone)
    case = ngc.parity_case(n)
    codes, margin = ngc.parity_codes(case)
    assert margin > 1e-12
    ref = ngc.parity_reference(n)
    eng = _engine(tq, n, case["psi0"], case["ham"], case["seed"], ngc.PARITY_T)
    _load(tq, eng, case["circuits"])
    f, g = _grad_run(eng)
    info = eng.device_info()
    if n == 13:
        assert case["batch"] > info["cu_count"] * info["wg_per_cu"]      # the grid is persistent: workgroups take several circuits
    off = _offsets(case["circuits"])
    for b in case["check"]:
        e_ref, g_ref = ref[b]
        gb = g[off[b]:off[b + 1]]
        print(f"n={n} b={b}: |E - E_ref| = {abs(f[b] - e_ref):.3e}, |g - g_ref|_inf = {np.abs(gb - g_ref).max():.3e}, "
              f"errors per realisation {[int(np.count_nonzero(c)) for c in codes[b]]}")
        assert abs(f[b] - e_ref) <= TOL * case["scale"], (n, b, f[b], e_ref)
        assert np.abs(gb - g_ref).max() <= TOL * case["scale"], (n, b)
    assert eng.noise_grad_info() == {"n_real": ngc.PARITY_T, "hold": False, "eval_base": ngc.PARITY_T}
    eng.close()


def test_one_e_t_is_the_mean_of_the_energy_runs(tq):
    """E_T of energy_grad_batch at B parameter vectors = the mean of the T values energy_batch returns for the same
    counters (two engines with the same seed: energy_batch moves the counter by one per call)."""
    n, T, B = 9, 5, 4
    case = ngc.parity_case(n)
    g, th = case["circuits"][0]
    ths = np.stack([th + 0.1 * b for b in range(B)])
    a = _engine(tq, n, case["psi0"], case["ham"], 77, T)
    a.set_circuit(tq.Circuit(*g, th.size))
    e_t, _ = a.energy_grad_batch(ths)
    b = _engine(tq, n, case["psi0"], case["ham"], 77, 0)
    b.set_circuit(tq.Circuit(*g, th.size))
    es = np.stack([b.energy_batch(ths) for _ in range(T)])
    total = np.zeros(B)
    for t in range(T):
        total = total + es[t]
    assert np.abs(e_t - total / T).max() <= 1e-12 * case["scale"]
    assert np.ptp(es, axis=0).min() > 1e-6      # the T draws differ: the mean is one of several values
    a.close(), b.close()


def test_pauli_table(tq):
    """a biased, Z-heavy table in both slots (p1 / p2 of set_noise set to values the table must replace)"""
    n, T, seed = 4, 3, 4321
    w1 = np.array([0.02, 0.03, 0.25])
    w2 = np.full(15, 0.004)
    w2[[3 - 1, 12 - 1, 15 - 1]] = 0.08
    rng = np.random.default_rng(41)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 10, rng)
    circuits = []
    for _ in range(3):
        kind, q0, q1, pidx, th = random_gates(n, 40, rng, p_cnot=0.4)
        circuits.append((with_noise_gates(kind, q0, q1, pidx), th))
    eng = _engine(tq, n, psi0, ham, seed, T, p=(0.5, 0.5), tables=(w1, w2))
    _load(tq, eng, circuits)
    f, g = _grad_run(eng)
    off, sc, n_z = _offsets(circuits), ngc.scale(ham), 0
    for b, (gates, th) in enumerate(circuits):
        codes, margin = ngc.codes_of(seed, b, 0, T, gates[0], w1, w2, (0.5, 0.5))
        assert margin > 1e-12
        n_z += sum(int(np.count_nonzero(c == 3)) for c in codes)
        e_ref, g_ref = ngc.mean(psi0, gates, th, ham, codes)
        assert abs(f[b] - e_ref) <= TOL * sc and np.abs(g[off[b]:off[b + 1]] - g_ref).max() <= TOL * sc, b
    assert n_z >= 10
    eng.close()


def test_shared_and_unused_parameters(tq):
    """parameter 0 drives two gates, parameter 2 none: the shared entry is the sum of the two entries of the circuit with
    a parameter per gate (same gates, same draws), both clearly non-zero; the unused entry is 0."""
    c = shared_unused_case()
    kind, q0, q1, pidx = c["gates"]
    th, ham, psi0, n = c["theta"], c["ham"], c["psi0"], 5
    shared = [g for g in range(kind.size) if pidx[g] == 0]
    assert len(shared) == 2 and not np.any(pidx == 2)
    own = pidx.copy()
    own[shared[1]] = th.size
    th_own = np.concatenate([th, [th[0]]])
    T, seed = 4, 99
    res = []
    for pi, t in ((pidx, th), (own, th_own)):
        eng = _engine(tq, n, psi0, ham, seed, T)
        eng.set_circuit(tq.Circuit(*with_noise_gates(kind, q0, q1, pi), t.size))
        res.append(eng.energy_grad(t))
        eng.close()
    (e1, g1), (e2, g2) = res
    assert e1 == e2
    assert min(abs(g2[0]), abs(g2[-1])) > 1e-3
    assert abs(g1[0] - (g2[0] + g2[-1])) <= TOL * ngc.scale(ham)
    assert g1[2] == 0.0
    gates = with_noise_gates(kind, q0, q1, pidx)
    codes, _ = ngc.codes_of(seed, 0, 0, T, gates[0])
    e_ref, g_ref = ngc.mean(psi0, gates, th, ham, codes)
    assert abs(e1 - e_ref) <= TOL * ngc.scale(ham) and np.abs(g1 - g_ref).max() <= TOL * ngc.scale(ham)


# ---- 2. bits and the counter ----------------------------------------------------------------------------------------------------

def test_bits(tq):
    """the same (seed, eval_base, batch position, T) gives the same bits: run twice; a circuit alone in a batch padded so
    that it keeps its position; L-BFGS with maxfun = 1 returns the f of energy_grad at x0"""
    n, T = 10, 3
    case = ngc.parity_case(n)
    circuits = case["circuits"]
    runs = []
    for _ in range(2):
        eng = _engine(tq, n, case["psi0"], case["ham"], 5, T)
        _load(tq, eng, circuits)
        runs.append(_grad_run(eng))
        eng.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # position 2 in another batch: the short circuit in front of it twice
    other = [circuits[1], circuits[1], circuits[2]]
    eng = _engine(tq, n, case["psi0"], case["ham"], 5, T)
    _load(tq, eng, other)
    f, g = _grad_run(eng)
    off_a, off_b = _offsets(circuits), _offsets(other)
    assert f[2] == runs[0][0][2] and np.array_equal(g[off_b[2]:], runs[0][1][off_a[2]:])
    # ... and its position matters
    _load(tq, eng, [circuits[2]])
    eng.set_noise(*P, 5)
    assert _grad_run(eng)[0][0] != runs[0][0][2]
    # L-BFGS, maxfun = 1: one evaluation at x0 on the same realisations
    eng.set_noise(*P, 5)
    _load(tq, eng, circuits)
    eng.batch_run_minimize_lbfgs(maxfun=1)
    x, f1, nfev = eng.batch_fetch()
    assert np.array_equal(f1, runs[0][0]) and np.all(nfev == 1)
    assert np.array_equal(x, np.concatenate([th for _, th in circuits]))
    eng.close()


def test_counter(tq):
    n, T = 4, 3
    rng = np.random.default_rng(8)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 8, rng)
    kind, q0, q1, pidx, th = random_gates(n, 12, rng, p_cnot=0.4)
    circuits = [(with_noise_gates(kind, q0, q1, pidx), th)] * 2
    eng = _engine(tq, n, psi0, ham, 11, T)
    info = lambda: eng.noise_grad_info()["eval_base"]
    assert eng.noise_grad_info() == {"n_real": T, "hold": False, "eval_base": 0}
    _load(tq, eng, circuits)
    r0 = _grad_run(eng)
    assert info() == T
    r1 = _grad_run(eng)
    assert info() == 2 * T and not np.array_equal(r0[1], r1[1])
    eng.batch_run_minimize_lbfgs(maxfun=3)
    assert info() == 3 * T
    eng.batch_set_new_gate([kind.size * 2 - 2, -1])
    eng.batch_run_env_step_lbfgs(maxfun=3)
    assert info() == 4 * T + 1
    eng.batch_set_new_gate(None)
    eng.batch_run_energy()
    assert info() == 4 * T + 2
    # hold: two gradient calls see the same function; advance moves on
    eng.set_noise(*P, 11)
    eng.set_noise_grad(T, hold=True)
    assert eng.noise_grad_info() == {"n_real": T, "hold": True, "eval_base": 0}
    h0 = _grad_run(eng)
    h1 = _grad_run(eng)
    assert info() == 0 and np.array_equal(h0[0], h1[0]) and np.array_equal(h0[1], h1[1])
    assert np.array_equal(h0[1], r0[1])                     # ... the one of the first run above
    eng.noise_grad_advance()
    assert info() == T
    h2 = _grad_run(eng)
    assert np.array_equal(h2[1], r1[1]) and not np.array_equal(h2[1], h0[1])
    eng.batch_run_minimize_lbfgs(maxfun=2)                  # L-BFGS moves the counter whatever hold is
    assert info() == 2 * T
    eng.close()


# ---- 3. L-BFGS ------------------------------------------------------------------------------------------------------------------

def _lbfgs_case():
    n = 6
    rng = np.random.default_rng(66)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 10, rng)
    circuits = []
    for _ in range(3):
        kind, q0, q1, pidx, th = random_gates(n, 14, rng, p_cnot=0.35)
        circuits.append((with_noise_gates(kind, q0, q1, pidx), th.astype(np.float32).astype(np.float64)))
    return n, psi0, ham, circuits


def test_lbfgs_descends_on_the_frozen_realisations(tq):
    n, psi0, ham, circuits = _lbfgs_case()
    T, seed, sc = 8, 321, None
    sc = ngc.scale(ham)
    eng = _engine(tq, n, psi0, ham, seed, T, p=(0.05, 0.08))
    _load(tq, eng, circuits)
    eng.batch_run_minimize_lbfgs(maxfun=60)
    x, f, nfev = eng.batch_fetch()
    off = _offsets(circuits)
    for b, (gates, th) in enumerate(circuits):
        codes, margin = ngc.codes_of(seed, b, 0, T, gates[0], p=(0.05, 0.08))
        assert margin > 1e-12
        f0 = ngc.mean(psi0, gates, th, ham, codes, want_grad=False)[0]
        f_end = ngc.mean(psi0, gates, x[off[b]:off[b + 1]], ham, codes, want_grad=False)[0]
        print(f"b={b}: f(x0) = {f0:.6f}, f_end = {f[b]:.6f}, oracle at x = {f_end:.6f}, nfev = {nfev[b]}")
        assert f[b] <= f0 + TOL * sc and nfev[b] > 1
        assert abs(f[b] - f_end) <= TOL * sc
    assert any(f[b] < ngc.mean(psi0, g, th, ham, ngc.codes_of(seed, b, 0, T, g[0], p=(0.05, 0.08))[0], want_grad=False)[0] - 1e-3
               for b, (g, th) in enumerate(circuits))
    assert eng.noise_grad_info()["eval_base"] == T
    eng.close()


def test_env_step_lbfgs_closing_energy(tq):
    """the optimiser runs on the pre-action circuit (the new gate and its noise gate left out, draws numbered by position
    in that list) with ids base .. base + T - 1; the closing energy is the single draw of id base + T on the full circuit
    at the float32-rounded parameters"""
    n, psi0, ham, circuits = _lbfgs_case()
    T, seed, sc, p = 4, 654, ngc.scale(ham), (0.05, 0.08)
    new = []
    for b, (gates, th) in enumerate(circuits):
        rot = [g for g in range(gates[0].size) if gates[3][g] >= 0]
        cn = [g for g in range(gates[0].size) if gates[0][g] == 0]
        new.append([rot[-1], cn[0], -1][b])
        if b == 0:
            th[gates[3][rot[-1]]] = 0.0
    eng = _engine(tq, n, psi0, ham, seed, T, p=p)
    _load(tq, eng, circuits)
    eng.batch_run_energy()                                   # the counter stands at 1
    base = 1
    eng.batch_set_new_gate(new)
    eng.batch_run_env_step_lbfgs(maxfun=25)
    x, f, nfev = eng.batch_fetch()
    xraw = eng.batch_fetch_xopt()
    off = _offsets(circuits)
    for b, (gates, th) in enumerate(circuits):
        kind, q0, q1, pidx = gates
        xb = x[off[b]:off[b + 1]]
        assert np.array_equal(xb, xraw[off[b]:off[b + 1]].astype(np.float32).astype(np.float64))
        codes, m = npo.draws(seed, b, base + T, kind, None, None, *p)
        assert m > 1e-12
        ref = ngc.energy(psi0, gates, xb, ham, codes)
        assert abs(f[b] - ref) <= TOL * sc, (b, f[b], ref)
        # the optimiser did not go up on its own function: the pre-action circuit, ids base .. base + T - 1
        keep = np.ones(kind.size, bool)
        hole = -1
        if new[b] >= 0:
            keep[new[b]] = keep[new[b] + 1] = False
            hole = int(pidx[new[b]])
        pre = (kind[keep], q0[keep], q1[keep], pidx[keep])
        pcodes, m = ngc.codes_of(seed, b, base, T, pre[0], p=p)
        assert m > 1e-12
        f0 = ngc.mean(psi0, pre, th, ham, pcodes, want_grad=False)[0]
        fx = ngc.mean(psi0, pre, xraw[off[b]:off[b + 1]], ham, pcodes, want_grad=False)[0]
        assert fx <= f0 + TOL * sc, (b, fx, f0)
        if hole >= 0:
            assert xraw[off[b] + hole] == th[hole]
    assert eng.noise_grad_info()["eval_base"] == base + T + 1
    eng.close()


# ---- 4. statistics --------------------------------------------------------------------------------------------------------------

def test_sampled_gradient_against_the_exact_channel(tq):
    """n = 3, one circuit at 64 positions, T = 64: the 64 block means give a mean and its sigma; every entry within
    4 sigma of the gradient of the exact channel mode (vqe_set_dm_grad) - the project's bound for sampler against exact
    channel.  The CPU oracle alone satisfies it for this seed (asserted first)."""
    c = ngc.stat_case()
    ok, _, _ = ngc.within_4_sigma(ngc.stat_oracle_blocks(c), ngc.stat_exact_grad(c))
    assert ok
    circ = tq.Circuit(*c["gates"], c["theta"].size)
    ex = tq.VQEEngine(c["n"])
    ex.set_init_state(c["psi0"]), ex.set_hamiltonian(*c["ham"])
    ex.set_noise(*c["p"], 1)
    ex.set_noise_mode(1), ex.set_dm_batched(-1), ex.set_dm_grad(True)
    ex.set_circuit(circ)
    exact = ex.energy_grad(c["theta"])[1]
    ex.close()
    assert np.abs(exact - ngc.stat_exact_grad(c)).max() <= 1e-9
    eng = _engine(tq, c["n"], c["psi0"], c["ham"], c["seed"], ngc.STAT_T, p=c["p"])
    eng.set_circuit(circ)
    _, g = eng.energy_grad_batch(np.tile(c["theta"], (ngc.STAT_B, 1)))
    ok, m, s = ngc.within_4_sigma(g, exact)
    print("exact", exact, "mean", m, "sigma", s)
    assert ok
    assert np.abs(g - ngc.stat_oracle_blocks(c)).max() <= TOL * ngc.scale(c["ham"])
    eng.close()


# ---- 5. the switch off ----------------------------------------------------------------------------------------------------------

def test_switch_off_refusals_and_noiseless_bits(tq):
    n = 4
    rng = np.random.default_rng(2)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 8, rng)
    kind, q0, q1, pidx, th = random_gates(n, 12, rng, p_cnot=0.4)
    gates = with_noise_gates(kind, q0, q1, pidx)
    circ = tq.Circuit(*gates, th.size)
    # off (the default): refused as before, nothing changes
    eng = _engine(tq, n, psi0, ham, 3, 0)
    eng.set_circuit(circ)
    for call in (lambda: eng.energy_grad(th), lambda: eng.minimize_lbfgs(th, maxfun=3)):
        with pytest.raises(RuntimeError, match=rf"error {ESTATE}:.*Pauli-noise trajectories.*vqe_set_noise_grad"):
            call()
    assert eng.noise_grad_info() == {"n_real": 0, "hold": False, "eval_base": 0}
    # bad counts
    for bad in (-1, 4097):
        with pytest.raises(RuntimeError, match=rf"error {EINVAL}:"):
            eng.set_noise_grad(bad)
    # on, but what stays refused: shot noise, mode 1 without the exact gradient, a Kraus override, L-BFGS on a term shard
    eng.set_noise_grad(4)
    eng.set_shot_noise(0.1, 3)
    with pytest.raises(RuntimeError, match=rf"error {ESTATE}:.*shot noise"):
        eng.energy_grad(th)
    eng.set_shot_noise(0.0, 3)
    eng.set_noise_mode(1)
    with pytest.raises(RuntimeError, match=rf"error {ESTATE}:"):
        eng.energy_grad(th)
    eng.set_noise_mode(0)
    eng.set_noise_kraus(tq.channels.amplitude_damping(0.1), None)
    with pytest.raises(RuntimeError, match=rf"error {ESTATE}:.*Kraus"):
        eng.energy_grad(th)
    eng.set_kraus_traj(4)
    with pytest.raises(RuntimeError, match=rf"error {ESTATE}:.*Kraus"):
        eng.energy_grad(th)
    eng.set_kraus_traj(0)
    eng.set_noise_kraus(None, None)
    eng.set_term_shard(0, 2)
    with pytest.raises(RuntimeError, match=rf"error {ESTATE}:.*term-sharded"):
        eng.minimize_lbfgs(th, maxfun=3)
    e0, g0 = eng.energy_grad(th)                             # the gradient of a term shard is served: a partial E_T
    assert eng.noise_grad_info()["eval_base"] == 4           # the refused calls above moved nothing
    eng.set_term_shard(1, 2)
    eng.set_noise(*P, 3)
    e1, g1 = eng.energy_grad(th)
    eng.set_term_shard(0, 1)
    eng.set_noise(*P, 3)
    e, g = eng.energy_grad(th)
    sc = ngc.scale(ham)
    assert abs(e0 + e1 - e) <= 1e-12 * sc and np.abs(g0 + g1 - g).max() <= 1e-12 * sc
    eng.close()
    # on and no noise: the noiseless kernels, bit for bit what an engine that never heard of the switch returns
    res = []
    for T in (0, 16):
        eng = _engine(tq, n, psi0, ham, 3, T, p=(0.0, 0.0))
        eng.set_circuit(circ)
        res.append((eng.energy_grad(th), eng.minimize_lbfgs(th, maxfun=20), eng.noise_grad_info()["eval_base"]))
        eng.close()
    (a_g, a_l, a_c), (b_g, b_l, b_c) = res
    assert a_g[0] == b_g[0] and np.array_equal(a_g[1], b_g[1])
    assert np.array_equal(a_l[0], b_l[0]) and a_l[1:] == b_l[1:]
    assert a_c == b_c == 0


def test_n14_is_refused_with_the_switch_on(tq):
    eng = tq.VQEEngine(14)
    eng.set_noise(*P, 1)
    eng.set_noise_grad(2)
    eng.set_stream_grad(True)
    eng.set_circuit(tq.Circuit(np.array([1, 4], np.int32), np.array([0, 0], np.int32), np.array([-1, -1], np.int32),
                               np.array([0, -1], np.int32), 1))
    zs = np.array([1], np.uint64)
    eng.set_hamiltonian(np.array([0], np.uint64), zs, np.array([1.0]))
    with pytest.raises(RuntimeError, match=rf"error {ESTATE}:.*Pauli-noise trajectories.*n_qubits <= 13"):
        eng.energy_grad(np.array([0.3]))
    assert eng.noise_grad_info()["eval_base"] == 0
    eng.close()


# ---- 6. environments ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    from helpers import make_data_root
    return make_data_root(str(tmp_path_factory.mktemp("dmrg-to-qc")))


def test_vec_env_lbfgs_on_frozen_realisations(data_root):
    """the 8-qubit noisy fixture, 4 environments, T = 4: the compiled host loop and the Python one agree bit for bit, and
    every step's energy is the oracle's single draw of id eval_base + T on the full circuit at the committed angles"""
    import torch
    from helpers import reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2_noise", data_root)
    conf["non_local_opt"]["global_iters"] = 30
    dev = torch.device("cuda:0")
    B, T, seed = 4, 4, 4
    with pytest.raises(NotImplementedError):                  # without noise_realisations: as before
        VecCircuitEnv(CircuitEnv, conf, dev, B, seed=seed, device_optimizer="lbfgs")
    with pytest.raises(ValueError):
        VecCircuitEnv(CircuitEnv, conf, dev, B, seed=seed, noise_realisations=T)
    vn = VecCircuitEnv(CircuitEnv, conf, dev, B, seed=seed, native=True, device_optimizer="lbfgs", noise_realisations=T)
    vp = VecCircuitEnv(CircuitEnv, conf, dev, B, seed=seed, native=False, device_optimizer="lbfgs", noise_realisations=T)
    assert vn.native and not vp.native
    assert torch.equal(vn.reset(), vp.reset())
    for v in (vn, vp):                                        # align the counters (the Python reset evaluates B energies)
        v.engine.set_noise(CircuitEnv.NOISE_P1, CircuitEnv.NOISE_P2, seed)
    p = (CircuitEnv.NOISE_P1, CircuitEnv.NOISE_P2)
    proto = vp.envs[0]
    ham = (np.asarray(proto.ham.xmask, np.uint64), np.asarray(proto.ham.zmask, np.uint64), np.asarray(proto.ham.coeff, np.float64))
    sc = ngc.scale(ham)
    table = proto._actions_table
    rng = np.random.default_rng(23)
    for t in range(4):
        base = vp.engine.noise_grad_info()["eval_base"]
        assert base == vn.engine.noise_grad_info()["eval_base"] == t * (T + 1)
        ill = vp.illegal_actions()
        acts = []
        for b in range(B):
            a = int(rng.integers(len(table)))
            while a in ill[b]:
                a = int(rng.integers(len(table)))
            acts.append(table[a])
        on, rn, dn = vn.step(acts)
        op, rp, dp = vp.step(acts)
        assert torch.equal(on, op) and torch.equal(rn, rp) and dn == dp, t
        for b in range(B):
            e, w = vp.envs[b], vn.envs[b]
            assert (w.energy, w.error, w.nfev) == (e.energy, e.error, e.nfev) and torch.equal(w.state, e.state)
            circ, ang = e._circuit(e.state)
            gates = (np.asarray(circ.kind), np.asarray(circ.q0), np.asarray(circ.q1), np.asarray(circ.pidx))
            codes, margin = npo.draws(seed, b, base + T, gates[0], None, None, *p)
            assert margin > 1e-12
            ref = ngc.energy(proto.TN_state, gates, np.asarray(ang, np.float64), ham, codes)
            assert abs(float(e.energy) - ref) <= TOL * sc, (t, b, float(e.energy), ref)
        assert not any(dn)
    vn.close()


def test_circuit_env_scipy_gradient_method_on_a_noisy_class(data_root):
    """optim_alg = L-BFGS-B on the noisy class: refused without non_local_opt.noise_realisations; with it two steps run,
    the counter moves by T + 1 per step (T held during scipy, one draw for the step's energy)"""
    import torch
    from helpers import reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2_noise", data_root)
    conf["non_local_opt"]["global_iters"] = 15
    conf["non_local_opt"]["optim_alg"] = "L-BFGS-B"
    dev = torch.device("cuda:0")
    with pytest.raises(NotImplementedError, match="noise_realisations"):
        CircuitEnv(conf, dev, seed=5)
    T = 4
    conf["non_local_opt"]["noise_realisations"] = T
    env = CircuitEnv(conf, dev, seed=5)
    env.reset()
    assert env.engine.noise_grad_info()["n_real"] == T and env.engine.noise_grad_info()["hold"]
    table = env._actions_table
    for k, ai in enumerate((3, 60)):
        base = env.engine.noise_grad_info()["eval_base"]
        obs, rwd, done = env.step(table[ai])
        assert env.engine.noise_grad_info()["eval_base"] == base + T + 1
        assert env.min_eig - 1e-9 <= env.energy <= env.max_eig + 1e-9 and torch.isfinite(rwd)
        assert env.nfev >= 1
