"""GPU: quantum-jump trajectories of a Kraus channel in mode 0 (vqe_set_kraus_traj, csrc/vqe_qjump.h).

Reference: tests/qj_oracle.py, a physical-frame state-vector simulation with the selection rule of include/vqe_hip.h
(tied to the exact channel and to the C oracle's Pauli path by tests/test_kraus_traj_cpu.py).  Tolerances: every
energy 1e-10 max(1, sum |c_k|), amplitudes 1e-12 (the project's A_TOL); the distribution test 5 sem + 1e-12, the margin
of test_noise_statistics_match_depolarizing_channels, sem from the oracle's sample.  The parity test's two
preconditions - every draw at least 1e-9 from a boundary, every Kraus index chosen - are asserted on the oracle alone."""
import numpy as np
import pytest

import dm_kraus_oracle as ko
import qj_cases as qc
import qj_oracle as qo

pytestmark = pytest.mark.gpu
TOL = 1e-10
A_TOL = 1e-12
ESTATE, EINVAL = -1, -22
P1, P2 = 0.03, 0.07      # the depolarising channels of a slot without an override


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


def _engine(tq, n, psi0, ham, K1, K2, T, seed, p=(P1, P2), mode=0):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(p[0], p[1], seed)
    eng.set_noise_mode(mode)
    if K1 is not None or K2 is not None:
        eng.set_noise_kraus(K1, K2)
    eng.set_kraus_traj(T)
    return eng


def _circ(tq, c):
    return tq.Circuit(c[0], c[1], c[2], c[3], c[4].size)


def _load(tq, eng, circuits, thetas=None):
    eng.batch_load([_circ(tq, c) for c in circuits], [c[4] for c in circuits] if thetas is None else thetas)


# ---- 1. per-trajectory parity -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", qc.COMBOS)
@pytest.mark.parametrize("n", qc.PARITY_N)
def test_per_trajectory_parity(tq, n, name):
    psi0, ham, circuits = qc.parity_case(n)
    K1, K2 = qc.combo(name)
    T, B = qc.PARITY_T, len(circuits)
    runs = qc.oracle_runs(psi0, ham, circuits, K1, K2, qc.PARITY_SEED, qc.PARITY_EVALS, T)
    qc.assert_preconditions(runs, K1, K2)
    eng = _engine(tq, n, psi0, ham, K1, K2, T, qc.PARITY_SEED)
    _load(tq, eng, circuits)
    scale = _scale(ham)
    for e in range(qc.PARITY_EVALS):
        eng.batch_run_energy()
        f = eng.batch_fetch(want_x=False)[1]
        et = eng.batch_fetch_traj()
        info = eng.kraus_traj_info()
        want = np.array([r["energies"] for r in runs[e]])
        print(f"n={n} {name} evaluation {e}: max |dE_t| = {np.abs(et - want).max():.2e}, jumps {info['jumps']} "
              f"(oracle {sum(r['jumps'] for r in runs[e])}), workgroups {info['workgroups']}")
        assert et.shape == (B, T) and np.abs(et - want).max() <= TOL * scale, (e, et, want)
        for b in range(B):
            s = 0.0
            for v in et[b]:
                s += float(v)
            assert f[b] == s / T                                          # the mean, summed in t order
            assert abs(f[b] - runs[e][b]["mean"]) <= TOL * scale
        assert info["n_traj"] == T and info["evaluations"] == 1 and 1 <= info["workgroups"] <= B * T
        assert info["jumps"] == sum(r["jumps"] for r in runs[e])
    # the state of trajectory 0 at the counter (stream 0, evaluation 3)
    c = circuits[0]
    eng.set_circuit(_circ(tq, c))
    psi = eng.get_state(c[4])
    ref = qo.run(psi0, c[0], c[1], c[2], c[3], c[4], K1, K2, ham, qc.PARITY_SEED, 0, qc.PARITY_EVALS, 1)
    print(f"n={n} {name}: state max |d amp| = {np.abs(psi - ref['states'][0]).max():.2e}")
    assert np.abs(psi - ref["states"][0]).max() <= A_TOL
    assert abs(np.linalg.norm(psi) - 1.0) <= A_TOL
    # ... which advanced the counter: an energy draws at evaluation 4
    e4 = eng.energy(c[4])
    r4 = qo.run(psi0, c[0], c[1], c[2], c[3], c[4], K1, K2, ham, qc.PARITY_SEED, 0, qc.PARITY_EVALS + 1, T)
    assert abs(e4 - r4["mean"]) <= TOL * scale
    assert np.abs(eng.batch_fetch_traj() - r4["energies"][None, :]).max() <= TOL * scale


def test_depolarising_slot_without_an_override_and_an_identity_slot(tq):
    """n1 == 0: the one-qubit slot runs the depolarising Kraus set of p1; p2 = 0 without a K2: that slot is skipped"""
    n = 5
    psi0, ham, circuits = qc.parity_case(n)
    K2 = qc.combo("dephasing+cnot")[1]
    for K1o, K2o, p, K1r, K2r in ((None, K2, (0.2, 0.0), ko.depol1(0.2), K2), (qc.amplitude_damping(0.3), None, (0.0, 0.0), qc.amplitude_damping(0.3), None),
                                  (qc.amplitude_damping(0.3), None, (0.0, 0.3), qc.amplitude_damping(0.3), ko.depol2(0.3))):
        eng = _engine(tq, n, psi0, ham, K1o, K2o, 4, 77, p=p)
        _load(tq, eng, circuits)
        eng.batch_run_energy()
        want = np.array([r["energies"] for r in qc.oracle_runs(psi0, ham, circuits, K1r, K2r, 77, 1, 4)[0]])
        assert np.abs(eng.batch_fetch_traj() - want).max() <= TOL * _scale(ham)


def test_persistent_grid_and_shot_noise(tq):
    """B T beyond what the device holds: a workgroup runs several (circuit, trajectory) items, of more than one circuit;
    and the shot-noise term, once per evaluation: sigma * noise_gauss(seed, b, e) as the C oracle restates it."""
    import c_oracle as co
    n, T, seed, sigma = 5, 2048, 606, 0.37
    psi0, ham, circuits = qc.parity_case(n)
    K1, K2 = qc.combo("damping+product")
    scale = _scale(ham)
    eng = _engine(tq, n, psi0, ham, K1, K2, T, seed)
    eng.set_shot_noise(sigma, seed)
    _load(tq, eng, circuits)
    for e in range(2):
        eng.batch_run_energy()
        f = eng.batch_fetch(want_x=False)[1]
        et = eng.batch_fetch_traj()
        info = eng.kraus_traj_info()
        runs = qc.oracle_runs(psi0, ham, circuits, K1, K2, seed, 1, T, first_eval=e)[0]
        assert 1 <= info["workgroups"] < len(circuits) * T, info
        assert min(r["margin"] for r in runs) >= qc.MARGIN
        assert np.abs(et - np.array([r["energies"] for r in runs])).max() <= TOL * scale
        assert info["jumps"] == sum(r["jumps"] for r in runs)
        for b, r in enumerate(runs):
            assert abs(f[b] - (r["mean"] + sigma * co.lib().orc_noise_gauss(seed, b, e))) <= TOL * scale


# ---- 2. distribution ----------------------------------------------------------------------------------------------------

def test_mean_over_trajectories_is_the_exact_channel(tq):
    psi0, ham, c = qc.dist_case()
    K1, K2 = qc.combo("damping+product")
    exact = ko.circuit_energy(psi0, c[0], c[1], c[2], c[3], c[4], K1, K2, ham)
    runs = qc.oracle_runs(psi0, ham, [c], K1, K2, qc.DIST_SEED, qc.DIST_EVALS, qc.DIST_T)
    s = np.concatenate([r[0]["energies"] for r in runs])
    sem = s.std() / np.sqrt(s.size)
    eng = _engine(tq, 3, psi0, ham, K1, K2, qc.DIST_T, qc.DIST_SEED, p=(0.2, 0.4))
    eng.set_circuit(_circ(tq, c))
    means = np.array([eng.energy(c[4]) for _ in range(qc.DIST_EVALS)])
    mean = float(means.mean())
    print(f"device mean {mean:.8f} oracle mean {s.mean():.8f} exact {exact:.8f} sem {sem:.2e}")
    assert sem > 0 and abs(mean - exact) < 5 * sem + 1e-12, (mean, exact, sem)
    assert np.abs(means - np.array([r[0]["mean"] for r in runs])).max() <= TOL * _scale(ham)
    eng.set_noise_mode(1)                                                 # the engine's own exact channel on that handle
    e1 = eng.energy(c[4])
    assert abs(e1 - exact) <= TOL * _scale(ham) and abs(mean - e1) < 5 * sem


# ---- 3. optimisers ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 10])
def test_device_cobyla_and_env_step(tq, n):
    maxfun, T, seed = 25, 4, 31337
    psi0, ham, _ = qc.parity_case(n)
    rng = np.random.default_rng(8800 + n)
    circuits = [qc.noisy_su4(n, 9, rng) for _ in range(2)]
    K1, K2 = qc.combo("damping+product")
    scale = _scale(ham)
    eng = _engine(tq, n, psi0, ham, K1, K2, T, seed)
    _load(tq, eng, circuits)
    # env-step: the action added the last rotation of every circuit
    new_gate = [int(np.nonzero(c[3] >= 0)[0][-1]) for c in circuits]
    eng.batch_set_new_gate(new_gate)
    eng.batch_run_env_step(1.0, 1e-4, maxfun)                             # counter 0: the final evaluation is maxfun + 1
    x, f, nfev = eng.batch_fetch()
    et = eng.batch_fetch_traj()
    off = 0
    for b, c in enumerate(circuits):
        xb = x[off:off + c[4].size]
        off += c[4].size
        assert np.array_equal(xb, xb.astype(np.float32).astype(np.float64))
        r = qo.run(psi0, c[0], c[1], c[2], c[3], xb, K1, K2, ham, seed, b, maxfun + 1, T)
        print(f"n={n} env-step circuit {b}: nfev={nfev[b]} f={f[b]:.10f} |df|={abs(f[b] - r['mean']):.2e}")
        assert abs(f[b] - r["mean"]) <= TOL * scale and np.abs(et[b] - r["energies"]).max() <= TOL * scale
        assert 1 <= nfev[b] <= maxfun
    assert eng.kraus_traj_info()["evaluations"] == nfev.max() + 1
    # minimise (counter maxfun + 1): some evaluation k = 1 .. nfev reproduces f at the returned x
    base = maxfun + 1
    eng.batch_set_new_gate(None)
    eng.batch_run_minimize(1.0, 1e-4, maxfun)
    x, f, nfev = eng.batch_fetch()
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
        eng.batch_fetch_traj()                                            # (a minimisation leaves no per-trajectory energies)
    off = 0
    for b, c in enumerate(circuits):
        xb = x[off:off + c[4].size]
        off += c[4].size
        d = [abs(f[b] - qo.run(psi0, c[0], c[1], c[2], c[3], xb, K1, K2, ham, seed, b, base + k, T)["mean"]) for k in range(1, nfev[b] + 1)]
        print(f"n={n} minimise circuit {b}: nfev={nfev[b]} f={f[b]:.10f} best k={1 + int(np.argmin(d))} |df|={min(d):.2e}")
        assert min(d) <= TOL * scale and 1 <= nfev[b] <= maxfun
    # a following energy run draws at the advanced counter
    eng.batch_run_energy()
    f = eng.batch_fetch(want_x=False)[1]
    for b, c in enumerate(circuits):
        r = qo.run(psi0, c[0], c[1], c[2], c[3], c[4], K1, K2, ham, seed, b, 2 * (maxfun + 1), T)
        assert abs(f[b] - r["mean"]) <= TOL * scale
    # the single-circuit entry point (stream 0)
    c = circuits[1]
    eng.set_noise(P1, P2, seed)
    eng.set_circuit(_circ(tq, c))
    xs, fs, ns = eng.minimize_cobyla(c[4], 1.0, 1e-4, maxfun)
    d = [abs(fs - qo.run(psi0, c[0], c[1], c[2], c[3], xs, K1, K2, ham, seed, 0, k, T)["mean"]) for k in range(1, ns + 1)]
    assert min(d) <= TOL * scale


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------

def test_same_bits_on_repeat_and_in_another_batch(tq):
    n, T, seed = 10, 8, 5150
    psi0, ham, circuits = qc.parity_case(n)
    rng = np.random.default_rng(1)
    others = [qc.noisy_su4(n, 7, rng), qc.noisy_su4(n, 30, rng)]
    K1, K2 = qc.combo("damping+product")
    eng = _engine(tq, n, psi0, ham, K1, K2, T, seed)
    _load(tq, eng, circuits)
    eng.batch_run_energy()
    a = eng.batch_fetch_traj().copy()
    eng.batch_run_energy()
    assert not np.array_equal(eng.batch_fetch_traj(), a)                  # (the next evaluation)
    eng.set_noise(P1, P2, seed)
    eng.batch_run_energy()
    assert np.array_equal(eng.batch_fetch_traj(), a)
    eng.set_noise(P1, P2, seed)
    _load(tq, eng, [others[0], circuits[1], others[1], circuits[0]])
    eng.batch_run_energy()
    assert np.array_equal(eng.batch_fetch_traj()[1], a[1])


# ---- 5. refusals and the switch ---------------------------------------------------------------------------------------------

def test_switch_and_refusals(tq):
    n, T, seed = 5, 4, 99
    psi0, ham, circuits = qc.parity_case(n)
    K1, K2 = qc.combo("damping+product")
    scale = _scale(ham)
    eng = _engine(tq, n, psi0, ham, K1, K2, 0, seed)
    c = circuits[0]
    eng.set_circuit(_circ(tq, c))
    for bad in (-1, 4097):
        with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:"):
            eng.set_kraus_traj(bad)
    assert eng.kraus_traj_info()["n_traj"] == 0
    _load(tq, eng, circuits)
    calls = (eng.batch_run_energy, lambda: eng.batch_run_minimize(1.0, 1e-4, 20), lambda: eng.batch_run_env_step(1.0, 1e-4, 20),
             lambda: eng.energy(c[4]), lambda: eng.minimize_cobyla(c[4], maxfun=20))
    for call in calls:      # T = 0: refused as before, code and text
        with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*Kraus channel \(vqe_set_noise_kraus\) has no Pauli-trajectory form"):
            call()
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*has no state vector"):
        eng.get_state(c[4])
    eng.set_kraus_traj(4096)
    eng.set_kraus_traj(T)
    eng.batch_run_energy()
    before = eng.batch_fetch(want_x=False)[1].copy()
    want = np.array([r["mean"] for r in qc.oracle_runs(psi0, ham, circuits, K1, K2, seed, 1, T)[0]])
    assert np.abs(before - want).max() <= TOL * scale
    refused = (eng.batch_run_energy_grad, lambda: eng.batch_run_minimize_lbfgs(maxiter=1), lambda: eng.batch_run_env_step_lbfgs(maxiter=1),
               eng.batch_run_reduction, lambda: eng.energy_grad(c[4]), lambda: eng.minimize_lbfgs(c[4], maxiter=1))
    for call in refused:
        with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
            call()
    assert np.array_equal(eng.batch_fetch(want_x=False)[1], before)
    assert np.abs(eng.batch_fetch_traj().mean(axis=1) - before).max() <= 1e-12 * scale
    eng.batch_run_energy()                                                # the counter: evaluation 1, not further
    want = np.array([r["mean"] for r in qc.oracle_runs(psi0, ham, circuits, K1, K2, seed, 1, T, first_eval=1)[0]])
    assert np.abs(eng.batch_fetch(want_x=False)[1] - want).max() <= TOL * scale
    # a sharded handle and n = 14: refused before anything is loaded
    sh = _engine(tq, n, psi0, ham, K1, K2, T, seed)
    sh.set_term_shard(0, 2)
    sh.set_circuit(_circ(tq, c))
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*sharded"):
        sh.energy(c[4])
    big = tq.VQEEngine(14)
    big.set_noise_kraus(K1, K2)
    big.set_kraus_traj(T)
    big.set_circuit(tq.Circuit(np.array([1, 4], np.int32), np.array([0, 0], np.int32), np.array([-1, -1], np.int32), np.array([0, -1], np.int32), 1))
    for call in (lambda: big.energy(np.array([0.3])), lambda: big.get_state(np.array([0.3]))):
        with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*n_qubits <= 13"):
            call()
    # mode 1 keeps its exact channel with the switch on
    eng.set_noise_mode(1)
    eng.set_dm_rot2(True)
    eng.set_circuit(_circ(tq, c))
    assert abs(eng.energy(c[4]) - ko.circuit_energy(psi0, c[0], c[1], c[2], c[3], c[4], K1, K2, ham)) <= TOL * scale
    eng.set_noise_mode(0)
    # removing the override restores a fresh handle's bits (Pauli trajectories at the counter of a new handle)
    eng.set_noise_kraus(None, None)
    eng.set_noise(P1, P2, seed)
    fresh = _engine(tq, n, psi0, ham, None, None, 0, seed)
    fresh.set_circuit(_circ(tq, c))
    assert eng.energy(c[4]) == fresh.energy(c[4]) and eng.energy(c[4]) == fresh.energy(c[4])
    assert np.array_equal(eng.get_state(c[4]), fresh.get_state(c[4]))
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
        eng.batch_fetch_traj()


# ---- 6. environments --------------------------------------------------------------------------------------------------------

def test_vec_env_on_trajectories(tmp_path_factory):
    """VecCircuitEnv(noisy class, noise_channel="trajectory", noise_kraus=(K1, K2), kraus_trajectories=4): both host loops
    agree, and every reported energy is the oracle's at the reported angles, at the env-step's final evaluation id."""
    import torch
    import vqe_oracle as vo
    from helpers import load_case, make_data_root, oracle_init_state, reference_config
    from tensorrl_qas_amd import channels as ch
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv as cls
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    data_root = make_data_root(str(tmp_path_factory.mktemp("dmrg-to-qc")))
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2_noise", data_root)
    maxfun = 30
    conf["non_local_opt"]["global_iters"] = maxfun
    dev = torch.device("cuda:0")
    B, T, seed = 2, 4, 4
    K = (ch.amplitude_damping(0.02), ch.tensor(ch.amplitude_damping(0.05), ch.dephasing(0.03)))
    with pytest.raises(ValueError, match="kraus_trajectories"):
        VecCircuitEnv(cls, conf, dev, B, seed=seed, noise_channel="exact", noise_kraus=K, kraus_trajectories=T)
    with pytest.raises(ValueError, match="kraus_trajectories"):
        VecCircuitEnv(cls, conf, dev, B, seed=seed, noise_kraus=K, kraus_trajectories=0)
    vn = VecCircuitEnv(cls, conf, dev, B, seed=seed, native=True, noise_channel="trajectory", noise_kraus=K, kraus_trajectories=T)
    vp = VecCircuitEnv(cls, conf, dev, B, seed=seed, native=False, noise_channel="trajectory", noise_kraus=K, kraus_trajectories=T)
    assert vn.native and not vp.native and vp.engine.kraus_traj_info()["n_traj"] == T
    assert torch.equal(vn.reset(), vp.reset())
    for v in (vn, vp):      # the noise counter of both engines back to 0 (the two loops reset in different calls)
        v.engine.set_noise(cls.NOISE_P1, cls.NOISE_P2, seed)
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
            assert (w.energy, w.nfev) == (e.energy, e.nfev) and 1 <= e.nfev <= maxfun
            c = vo.ansatz_from_state(e.state.numpy(), n, noise=True)
            r = qo.run(psi0, c[0], c[1], c[2], c[3], c[4], K[0], K[1], ham, seed, b, (t + 1) * (maxfun + 1), T)
            print(f"step {t} env {b}: nfev={e.nfev} E={e.energy:.10f} |dE|={abs(e.energy - r['mean']):.2e} jumps {r['jumps']}")
            assert abs(e.energy - r["mean"]) < 1e-10, (t, b, e.energy, r["mean"])
    assert np.abs(vp.engine.batch_fetch_traj().mean(axis=1) - np.array([vp.envs[b].energy for b in range(B)])).max() < 1e-12
