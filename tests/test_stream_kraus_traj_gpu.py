"""GPU: quantum-jump trajectories of a Kraus channel on the streaming path (n >= 14; vqe_set_stream_kraus_traj,
csrc/vqe_stream_qjump.h).

Reference: tests/qj_oracle.py on the cases of tests/qj_cases.py, as for the LDS-resident path
(tests/test_kraus_traj_gpu.py), whose tolerances these are: every energy 1e-10 max(1, sum |c_k|), amplitudes 1e-12.  The
cross-path tie compares two device paths, each within 1e-10 scale of the same trajectory: 2e-10 scale.  The parity test's
two preconditions - every draw at least 1e-9 from a boundary, every Kraus index chosen - are asserted on the oracle alone
(tests/test_stream_kraus_traj_cpu.py asserts them without a GPU).  An oracle run is computed once per process."""
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
STREAM_N = (14, 15)

_RUNS = {}


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


def _parity_runs(n, name):
    """the oracle on qc.parity_case(n) under combo `name`: [evaluation][circuit], made once"""
    if (n, name) not in _RUNS:
        psi0, ham, circuits = qc.parity_case(n)
        K1, K2 = qc.combo(name)
        _RUNS[(n, name)] = qc.oracle_runs(psi0, ham, circuits, K1, K2, qc.PARITY_SEED, qc.PARITY_EVALS, qc.PARITY_T)
    return _RUNS[(n, name)]


def _engine(tq, n, psi0, ham, K1, K2, T, seed, p=(P1, P2), resident=-1):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(p[0], p[1], seed)
    if K1 is not None or K2 is not None:
        eng.set_noise_kraus(K1, K2)
    eng.set_kraus_traj(T)
    if resident is not None:
        eng.set_stream_kraus_traj(resident)
    return eng


def _circ(tq, c):
    return tq.Circuit(c[0], c[1], c[2], c[3], c[4].size)


def _load(tq, eng, circuits, thetas=None):
    eng.batch_load([_circ(tq, c) for c in circuits], [c[4] for c in circuits] if thetas is None else thetas)


def _t_ordered_mean(row):
    s = 0.0
    for v in row:
        s += float(v)
    return s / len(row)


# ---- 1. per-trajectory parity -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", qc.COMBOS)
@pytest.mark.parametrize("n", STREAM_N)
def test_per_trajectory_parity(tq, n, name):
    psi0, ham, circuits = qc.parity_case(n)
    K1, K2 = qc.combo(name)
    T, B = qc.PARITY_T, len(circuits)
    runs = _parity_runs(n, name)
    qc.assert_preconditions(runs, K1, K2)
    eng = _engine(tq, n, psi0, ham, K1, K2, T, qc.PARITY_SEED)
    assert eng.stream_kraus_traj_info() == {"resident": 0, "chunks": 0, "rounds": 0, "sweeps": 0}
    _load(tq, eng, circuits)
    scale = _scale(ham)
    rounds = max(int(np.count_nonzero((c[0] == 4) | (c[0] == 5))) for c in circuits)
    for e in range(qc.PARITY_EVALS):
        eng.batch_run_energy()
        f = eng.batch_fetch(want_x=False)[1]
        et = eng.batch_fetch_traj()
        info = eng.kraus_traj_info()
        sinfo = eng.stream_kraus_traj_info()
        want = np.array([r["energies"] for r in runs[e]])
        print(f"n={n} {name} evaluation {e}: max |dE_t| = {np.abs(et - want).max():.2e}, jumps {info['jumps']} "
              f"(oracle {sum(r['jumps'] for r in runs[e])}), stream info {sinfo}")
        assert et.shape == (B, T) and np.abs(et - want).max() <= TOL * scale, (e, et, want)
        for b in range(B):
            assert f[b] == _t_ordered_mean(et[b])                         # the mean, summed in t order
            assert abs(f[b] - runs[e][b]["mean"]) <= TOL * scale
        assert info["n_traj"] == T and info["evaluations"] == 1 and info["workgroups"] >= 1
        assert info["jumps"] == sum(r["jumps"] for r in runs[e])
        assert sinfo["resident"] == B * T and sinfo["chunks"] == 1 and sinfo["rounds"] == rounds
        assert sinfo["sweeps"] >= 1 + 2 * rounds                          # the initial state, two sweeps per jump round, the rotations
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


# ---- 2. the LDS-resident path draws the same trajectories -------------------------------------------------------------------

def test_cross_path_tie(tq):
    """qc.parity_case(13) on an n = 13 handle (LDS path) and, with psi0 (x) |0> and qubit 13 untouched, on an n = 14 handle
    (streaming path): the same (b, e, t, g), so the same draws."""
    psi0, ham, circuits = qc.parity_case(13)
    K1, K2 = qc.combo("damping+product")
    T, seed = qc.PARITY_T, qc.PARITY_SEED
    scale = _scale(ham)
    small = _engine(tq, 13, psi0, ham, K1, K2, T, seed, resident=None)
    big = _engine(tq, 14, np.concatenate([psi0, np.zeros_like(psi0)]), ham, K1, K2, T, seed)
    assert small.device_info()["lds_path"] and not big.device_info()["lds_path"]
    _load(tq, small, circuits)
    _load(tq, big, circuits)
    for e in range(3):
        small.batch_run_energy()
        big.batch_run_energy()
        a, b = small.batch_fetch_traj(), big.batch_fetch_traj()
        print(f"evaluation {e}: max |dE_t| between the paths = {np.abs(a - b).max():.2e}")
        assert np.abs(a - b).max() <= 2 * TOL * scale
        assert small.kraus_traj_info()["jumps"] == big.kraus_traj_info()["jumps"]


# ---- 3. slots ---------------------------------------------------------------------------------------------------------------

def test_depolarising_slot_without_an_override_and_an_identity_slot(tq):
    """n1 == 0: the one-qubit slot runs the depolarising Kraus set of p1; p2 = 0 without a K2: that slot is skipped"""
    n = 14
    psi0, ham, circuits = qc.parity_case(n)
    K2 = qc.combo("dephasing+cnot")[1]
    for K1o, K2o, p, K1r, K2r in ((None, K2, (0.2, 0.0), ko.depol1(0.2), K2), (qc.amplitude_damping(0.3), None, (0.0, 0.0), qc.amplitude_damping(0.3), None),
                                  (qc.amplitude_damping(0.3), None, (0.0, 0.3), qc.amplitude_damping(0.3), ko.depol2(0.3))):
        eng = _engine(tq, n, psi0, ham, K1o, K2o, 4, 77, p=p)
        _load(tq, eng, circuits)
        eng.batch_run_energy()
        runs = qc.oracle_runs(psi0, ham, circuits, K1r, K2r, 77, 1, 4)[0]
        assert min(r["margin"] for r in runs) >= qc.MARGIN
        want = np.array([r["energies"] for r in runs])
        got = eng.batch_fetch_traj()
        print(f"slots n1={0 if K1o is None else len(K1o)} n2={0 if K2o is None else len(K2o)} p={p}: max |dE_t| = {np.abs(got - want).max():.2e}")
        assert np.abs(got - want).max() <= TOL * _scale(ham)
        assert eng.kraus_traj_info()["jumps"] == sum(r["jumps"] for r in runs)


# ---- 4. chunking and bits ---------------------------------------------------------------------------------------------------

def test_same_bits_whatever_the_chunks_on_repeat_and_in_another_batch(tq):
    import c_oracle as co
    n, T, seed, name = 14, qc.PARITY_T, qc.PARITY_SEED, "damping+product"
    psi0, ham, circuits = qc.parity_case(n)
    K1, K2 = qc.combo(name)
    scale = _scale(ham)
    want = np.array([r["energies"] for r in _parity_runs(n, name)[0]])
    total = len(circuits) * T
    assert total == 24
    got = {}
    for resident in (-1, 24, 5, 1):
        eng = _engine(tq, n, psi0, ham, K1, K2, T, seed, resident=resident)
        _load(tq, eng, circuits)
        eng.batch_run_energy()
        got[resident] = (eng.batch_fetch_traj().copy(), eng.batch_fetch(want_x=False)[1].copy(), eng.kraus_traj_info()["jumps"])
        R = total if resident < 0 else resident
        sinfo = eng.stream_kraus_traj_info()
        assert sinfo["resident"] == R and sinfo["chunks"] == -(-total // R), (resident, sinfo)
    a = got[-1][0]
    assert np.abs(a - want).max() <= TOL * scale
    for resident in (24, 5, 1):
        assert np.array_equal(got[resident][0], a) and np.array_equal(got[resident][1], got[-1][1]), resident
        assert got[resident][2] == got[-1][2]
    # `eng` is the handle with one resident state: the next evaluation, the repeat, another batch, other chunks again
    eng.batch_run_energy()
    assert not np.array_equal(eng.batch_fetch_traj(), a)                  # (the next evaluation)
    eng.set_noise(P1, P2, seed)
    eng.batch_run_energy()
    assert np.array_equal(eng.batch_fetch_traj(), a)
    rng = np.random.default_rng(1)
    others = [qc.noisy_su4(n, 7, rng), qc.noisy_su4(n, 30, rng)]
    eng.set_noise(P1, P2, seed)
    eng.set_stream_kraus_traj(7)
    _load(tq, eng, [others[0], circuits[1], others[1], circuits[0]])
    eng.batch_run_energy()
    assert np.array_equal(eng.batch_fetch_traj()[1], a[1])
    assert eng.stream_kraus_traj_info()["chunks"] == -(-4 * T // 7)
    # shot noise: once per evaluation, sigma * noise_gauss(seed, b, e) as the C oracle restates it
    sigma = 0.37
    eng.set_noise(P1, P2, seed)
    eng.set_shot_noise(sigma, seed)
    _load(tq, eng, circuits)
    for e in range(2):
        eng.batch_run_energy()
        f = eng.batch_fetch(want_x=False)[1]
        et = eng.batch_fetch_traj()
        if e == 0:
            assert np.array_equal(et, a)
        for b in range(len(circuits)):
            assert abs(f[b] - (_t_ordered_mean(et[b]) + sigma * co.lib().orc_noise_gauss(seed, b, e))) <= TOL * scale


# ---- 5. optimisers ----------------------------------------------------------------------------------------------------------

def test_device_cobyla_and_env_step(tq):
    n, maxfun, T, seed = 14, 12, 2, 31337
    psi0, ham, _ = qc.parity_case(n)
    rng = np.random.default_rng(8800 + n)
    circuits = [qc.noisy_su4(n, 9, rng) for _ in range(2)]
    K1, K2 = qc.combo("damping+product")
    scale = _scale(ham)
    eng = _engine(tq, n, psi0, ham, K1, K2, T, seed, resident=3)          # two chunks per evaluation
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
        print(f"env-step circuit {b}: nfev={nfev[b]} f={f[b]:.10f} |df|={abs(f[b] - r['mean']):.2e}")
        assert abs(f[b] - r["mean"]) <= TOL * scale and np.abs(et[b] - r["energies"]).max() <= TOL * scale
        assert 1 <= nfev[b] <= maxfun
    assert eng.kraus_traj_info()["evaluations"] == nfev.max() + 1
    assert eng.stream_kraus_traj_info()["chunks"] == 2
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
        print(f"minimise circuit {b}: nfev={nfev[b]} f={f[b]:.10f} best k={1 + int(np.argmin(d))} |df|={min(d):.2e}")
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


# ---- 6. the switch and refusals ---------------------------------------------------------------------------------------------

def test_switch_and_refusals(tq):
    n, T, seed = 14, 2, 99
    psi0, ham, _ = qc.parity_case(n)
    rng = np.random.default_rng(6)
    circuits = [qc.noisy_su4(n, 7, rng) for _ in range(2)]
    K1, K2 = qc.combo("damping+product")
    scale = _scale(ham)
    c = circuits[0]
    eng = _engine(tq, n, psi0, ham, K1, K2, T, seed, resident=None)
    eng.set_circuit(_circ(tq, c))
    _load(tq, eng, circuits)
    off = (eng.batch_run_energy, lambda: eng.batch_run_minimize(1.0, 1e-4, 5), lambda: eng.batch_run_env_step(1.0, 1e-4, 5),
           lambda: eng.energy(c[4]), lambda: eng.get_state(c[4]), lambda: eng.minimize_cobyla(c[4], maxfun=5))
    for call in off:        # the switch off (the default, and 0): refused as before, code and text
        with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*n_qubits <= 13"):
            call()
    eng.set_stream_kraus_traj(0)
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*n_qubits <= 13"):
        eng.energy(c[4])
    with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:"):
        eng.set_stream_kraus_traj(-2)
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:.*n_qubits <= 13"):
        eng.energy(c[4])                                                  # (a refused setter leaves the switch off)
    assert eng.stream_kraus_traj_info() == {"resident": 0, "chunks": 0, "rounds": 0, "sweeps": 0}
    eng.set_stream_kraus_traj(-1)
    _load(tq, eng, circuits)
    eng.batch_run_energy()                                                # counter 0: every refused call left it alone
    before = eng.batch_fetch(want_x=False)[1].copy()
    traj = eng.batch_fetch_traj().copy()
    runs = qc.oracle_runs(psi0, ham, circuits, K1, K2, seed, 2, T)
    assert np.abs(before - np.array([r["mean"] for r in runs[0]])).max() <= TOL * scale
    refused = (eng.batch_run_energy_grad, lambda: eng.batch_run_minimize_lbfgs(maxiter=1), lambda: eng.batch_run_env_step_lbfgs(maxiter=1),
               eng.batch_run_reduction, lambda: eng.energy_grad(c[4]), lambda: eng.minimize_lbfgs(c[4], maxiter=1))
    for call in refused:
        with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
            call()
    for setup, undo in ((lambda: eng.set_term_shard(0, 2), lambda: eng.set_term_shard(0, 1)),
                        (lambda: eng.set_amplitude_shard(0, 2), lambda: eng.set_amplitude_shard(0, 1))):
        setup()
        for call in (eng.batch_run_energy, lambda: eng.batch_run_minimize(1.0, 1e-4, 5), lambda: eng.batch_run_env_step(1.0, 1e-4, 5)):
            with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
                call()
        undo()
    assert np.array_equal(eng.batch_fetch(want_x=False)[1], before)
    assert np.array_equal(eng.batch_fetch_traj(), traj)
    eng.batch_run_energy()                                                # the counter: evaluation 1, not further
    assert np.abs(eng.batch_fetch(want_x=False)[1] - np.array([r["mean"] for r in runs[1]])).max() <= TOL * scale
    with pytest.raises(tq.VQEError, match=rf"error {EINVAL}:"):
        eng.set_noise_mode(1)                                             # no density matrix at n = 14, as before
    # n = 5: the switch changes no bit of an LDS-path trajectory run
    p5, h5, c5 = qc.parity_case(5)
    pair = [_engine(tq, 5, p5, h5, K1, K2, 4, seed, resident=r) for r in (None, -1)]
    for e5 in pair:
        _load(tq, e5, c5)
        e5.batch_run_energy()
    assert np.array_equal(pair[0].batch_fetch_traj(), pair[1].batch_fetch_traj())
    assert pair[1].stream_kraus_traj_info()["resident"] == 0 and pair[0].kraus_traj_info() == pair[1].kraus_traj_info()
    # removing the override restores a fresh handle's bits (Pauli trajectories at the counter of a new handle)
    eng.set_noise_kraus(None, None)
    eng.set_noise(P1, P2, seed)
    fresh = _engine(tq, n, psi0, ham, None, None, 0, seed, resident=None)
    fresh.set_circuit(_circ(tq, c))
    eng.set_circuit(_circ(tq, c))
    assert eng.energy(c[4]) == fresh.energy(c[4]) and eng.energy(c[4]) == fresh.energy(c[4])
    assert np.array_equal(eng.get_state(c[4]), fresh.get_state(c[4]))
    _load(tq, eng, circuits)
    _load(tq, fresh, circuits)
    eng.batch_run_energy()
    fresh.batch_run_energy()
    assert np.array_equal(eng.batch_fetch(want_x=False)[1], fresh.batch_fetch(want_x=False)[1])
    with pytest.raises(tq.VQEError, match=rf"error {ESTATE}:"):
        eng.batch_fetch_traj()


# ---- 7. environments --------------------------------------------------------------------------------------------------------

def test_vec_env_on_trajectories_at_14_qubits(tmp_path):
    """VecCircuitEnv(noisy class, noise_channel="trajectory", noise_kraus=(K1, K2), kraus_trajectories=2) on the 14-qubit
    chain switches the streaming path's trajectories on for its engine: both host loops agree, and every reported energy
    is the oracle's at the reported angles, at the env-step's final evaluation id."""
    import torch
    import vqe_oracle as vo
    from tensorrl_qas_amd import channels as ch
    from tensorrl_qas_amd import synthetic
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv as cls
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    n, B, T, seed, maxfun = 14, 2, 2, 4, 6
    bound = float(3 * (n - 1) + n)
    conf = synthetic.write_chain_dataset(str(tmp_path / "dmrg-to-qc"), n, eigvals=[-bound, bound])
    conf["non_local_opt"]["global_iters"] = maxfun
    dev = torch.device("cuda:0")
    K = (ch.amplitude_damping(0.02), ch.tensor(ch.amplitude_damping(0.05), ch.dephasing(0.03)))
    with pytest.raises(Exception, match=rf"error {EINVAL}:"):             # no density matrix at 14 qubits, as before
        VecCircuitEnv(cls, conf, dev, B, seed=seed, noise_channel="exact", noise_kraus=K)
    vn = VecCircuitEnv(cls, conf, dev, B, seed=seed, native=True, noise_channel="trajectory", noise_kraus=K, kraus_trajectories=T)
    vp = VecCircuitEnv(cls, conf, dev, B, seed=seed, native=False, noise_channel="trajectory", noise_kraus=K, kraus_trajectories=T)
    assert vn.native and not vp.native and vp.engine.kraus_traj_info()["n_traj"] == T
    assert not vp.engine.device_info()["lds_path"]
    assert torch.equal(vn.reset(), vp.reset())
    for v in (vn, vp):      # the noise counter of both engines back to 0 (the two loops reset in different calls)
        v.engine.set_noise(cls.NOISE_P1, cls.NOISE_P2, seed)
    env = vp.envs[0]
    ham = (env.ham.xmask, env.ham.zmask, env.ham.coeff)
    psi0 = vo.statevector_from_qasm(open(env.spec.init_circuit_path()).read())
    table = env._actions_table
    nq = n * (n - 1)
    scripts = [[nq + 3 * 3 + 1, 5 * (n - 1) + 0], [2 * (n - 1) + 1, nq + 5 * 3 + 0]]      # RY q3, CNOT; CNOT, RX q5
    for t in range(2):
        acts = [table[s[t]] for s in scripts]
        on, rn, dn = vn.step(acts)
        op, rp, dp = vp.step(acts)
        assert torch.equal(on, op) and torch.equal(rn, rp) and dn == dp, t
        for b in range(B):
            e, w = vp.envs[b], vn.envs[b]
            assert (w.energy, w.nfev) == (e.energy, e.nfev) and 1 <= e.nfev <= maxfun
            c = vo.ansatz_from_state(e.state.numpy(), n, noise=True)
            r = qo.run(psi0, c[0], c[1], c[2], c[3], c[4], K[0], K[1], ham, seed, b, (t + 1) * (maxfun + 1), T)
            print(f"step {t} env {b}: nfev={e.nfev} E={e.energy:.10f} |dE|={abs(e.energy - r['mean']):.2e} jumps {r['jumps']}")
            assert abs(e.energy - r["mean"]) <= TOL * _scale(ham), (t, b, e.energy, r["mean"])
    assert vp.engine.stream_kraus_traj_info()["resident"] == B * T
    assert np.abs(vp.engine.batch_fetch_traj().mean(axis=1) - np.array([vp.envs[b].energy for b in range(B)])).max() < 1e-12
