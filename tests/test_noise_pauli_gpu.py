"""GPU: Pauli channel tables of the mode 0 sampler (vqe_set_noise_pauli, csrc/noise_pauli.h).

Reference: tests/noise_pauli_oracle.py - the draw rule of include/vqe_hip.h with the Python hash of tests/qj_oracle.py,
the codes handed to vo.run_circuit(noise_draws=...).  Every energy is compared on the same draws, to 1e-10 Ha; every test
that compares draws first asserts that no u lies within 1e-12 of a threshold (there the rule is the comparison of two
doubles and needs no margin, but a margin keeps the test independent of how a sum was rounded).  Mode 1 and the
quantum-jump runs: against the explicit Kraus override channels.pauli_channel(w) to 1e-12 (the same operators through the
same code), and against tests/dm_kraus_oracle.py to 1e-10."""
import numpy as np
import pytest

import dm_kraus_oracle as dk
import noise_pauli_oracle as npo
import vqe_oracle as vo
from helpers import random_gates, random_hamiltonian, random_state, tie_free_gates, with_noise_gates

pytestmark = pytest.mark.gpu
E_TOL = 1e-10
A_TOL = 1e-12
MARGIN = 1e-12
ESTATE, EINVAL = -1, -22


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _engine(tq, n, psi0, ham, seed, w1, w2, p=(0.0, 0.0)):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(p[0], p[1], seed)
    eng.set_noise_pauli(w1, w2)
    return eng


def _noisy_circuits(n, B, G, rng, p_cnot=0.3):
    """B circuits of G gates with a noise gate behind every gate: ((kind, q0, q1, pidx), theta)"""
    out = []
    for _ in range(B):
        kind, q0, q1, pidx, th = random_gates(n, G, rng, p_cnot=p_cnot)
        out.append((with_noise_gates(kind, q0, q1, pidx), th))
    return out


def _load(tq, eng, circuits):
    eng.batch_load([tq.Circuit(*g, th.size) for g, th in circuits], [th for _, th in circuits])


def _check_energy_runs(tq, eng, psi0, ham, circuits, seed, w1, w2, p, runs, first_eval=0):
    """`runs` consecutive energy runs of the resident batch against the oracle; returns the smallest margin"""
    margin = np.inf
    for e in range(first_eval, first_eval + runs):
        eng.batch_run_energy()
        f = eng.batch_fetch(want_x=False)[1]
        for b, (g, th) in enumerate(circuits):
            codes, m = npo.draws(seed, b, e, g[0], w1, w2, *p)
            margin = min(margin, m)
            ref = npo.energy(psi0, g, th, ham, codes)
            assert abs(f[b] - ref) <= E_TOL, (e, b, f[b], ref)
    return margin


# ---- 1. the LDS-resident path: energies, the counter, states -----------------------------------------------------------------

@pytest.mark.parametrize("name", list(npo.TABLES))
@pytest.mark.parametrize("n", [3, 4, 10])
def test_lds_energies_and_state(tq, n, name):
    """72 gates + 72 noise gates per circuit: the patch wave walks three chunks of 64 gates and carries the X offset of
    the drawn errors from one into the next.  n = 10: the scheduled, canonical layout.  p1 / p2 of set_noise are set to
    values the tables must replace."""
    w1, w2 = npo.TABLES[name]
    B, seed = (8 if n < 10 else 4), 9000 + n
    rng = np.random.default_rng(100 + n)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 20, rng)
    circuits = _noisy_circuits(n, B, 72, rng)
    eng = _engine(tq, n, psi0, ham, seed, w1, w2, p=(0.3, 0.3))
    assert eng.noise_pauli_info() == {"w1": True, "w2": True}
    _load(tq, eng, circuits)
    margin = _check_energy_runs(tq, eng, psi0, ham, circuits, seed, w1, w2, (0.3, 0.3), 3)
    # the state of stream 0 at the counter (evaluation 3), then an energy at evaluation 4
    g, th = circuits[1]
    eng.set_circuit(tq.Circuit(*g, th.size))
    codes, m3 = npo.draws(seed, 0, 3, g[0], w1, w2)
    psi = eng.get_state(th)
    assert np.abs(psi - npo.state(psi0, g, th, codes)).max() <= A_TOL
    codes, m4 = npo.draws(seed, 0, 4, g[0], w1, w2)
    assert abs(eng.energy(th) - npo.energy(psi0, g, th, ham, codes)) <= E_TOL
    assert min(margin, m3, m4) > MARGIN
    if name in ("distinct", "total_one"):      # most gates draw an error: the offset is carried across the chunks
        assert np.count_nonzero(codes) > (1 / 3 if name == "distinct" else 0.99) * (codes.size // 2)
    eng.close()


@pytest.mark.parametrize("which", ["w1_only", "w2_only"])
def test_one_slot_with_a_table_the_other_depolarising(tq, which):
    """a slot without a table keeps the floor rule of its p beside a table in the other slot"""
    n, seed, p = 4, 321, (0.25, 0.5)
    w1, w2 = npo.TABLES["distinct"]
    w1, w2 = (w1, None) if which == "w1_only" else (None, w2)
    rng = np.random.default_rng(7)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 20, rng)
    circuits = _noisy_circuits(n, 8, 72, rng)
    eng = _engine(tq, n, psi0, ham, seed, w1, w2, p=p)
    assert eng.noise_pauli_info() == {"w1": w1 is not None, "w2": w2 is not None}
    _load(tq, eng, circuits)
    assert _check_energy_runs(tq, eng, psi0, ham, circuits, seed, w1, w2, p, 2) > MARGIN
    eng.close()


# ---- 2. device COBYLA and the env-step ---------------------------------------------------------------------------------------

def test_cobyla_and_env_step_traces(tq):
    """n = 4, maxfun = 30: every traced evaluation of a minimisation is a run on the full gate list at counter + k, every
    traced evaluation of an env-step one on the PRE-action list (the new gate and its own noise gate left out and not
    counted), its final energy one on the full list at counter + maxfun + 1."""
    n, seed, maxfun = 4, 20250101, 30
    w1, w2 = npo.TABLES["distinct"]
    rng = np.random.default_rng(31)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 30, rng)
    raw, circs, ths, new = [], [], [], []
    for b in range(4):
        g = list(tie_free_gates(n, 5 + b, rng))
        g[4] = g[4].astype(np.float32).astype(np.float64)
        G = g[0].size
        ng = [G - 1, 0, G // 2, -1][b]
        if ng >= 0 and g[0][ng] != 0:
            g[4][g[3][ng]] = 0.0
        kind, q0, q1, pidx = with_noise_gates(*g[:4])
        raw.append((kind, q0, q1, pidx, g[4], ng))
        new.append(2 * ng if ng >= 0 else -1)
        circs.append(tq.Circuit(kind, q0, q1, pidx, g[4].size)), ths.append(g[4])
    eng = _engine(tq, n, psi0, ham, seed, w1, w2)
    eng.batch_set_trace(True)
    eng.batch_load(circs, ths)
    margin = np.inf
    # the minimisation: evaluation k (from 1) of stream b draws at counter 0 + k
    eng.batch_run_minimize(1.0, 1e-4, maxfun)
    _, _, nfev = eng.batch_fetch()
    for b, (kind, q0, q1, pidx, th, _) in enumerate(raw):
        ft, xt = eng.batch_fetch_trace(b, th.size)
        assert 1 <= nfev[b] <= maxfun
        for k in range(int(nfev[b])):
            codes, m = npo.draws(seed, b, k + 1, kind, w1, w2)
            margin = min(margin, m)
            ref = npo.energy(psi0, (kind, q0, q1, pidx), xt[k], ham, codes)
            assert abs(ft[k] - ref) <= E_TOL, ("minimize", b, k, ft[k], ref)
    # the env-step: the counter stands at maxfun + 1
    base = maxfun + 1
    eng.batch_set_new_gate(new)
    eng.batch_run_env_step(1.0, 1e-4, maxfun)
    x, f, nfev = eng.batch_fetch()
    off = 0
    for b, (kind, q0, q1, pidx, th, ng) in enumerate(raw):
        P = th.size
        xb = x[off:off + P]
        off += P
        keep = np.ones(kind.size, bool)
        hole = -1
        if ng >= 0:
            keep[2 * ng] = keep[2 * ng + 1] = False              # the gate and ITS noise channel
            if kind[2 * ng] != 0:
                hole = int(pidx[2 * ng])
        sel = [j for j in range(P) if j != hole]
        pk, pa, pb = kind[keep], q0[keep], q1[keep]
        pp = np.where(pidx[keep] > hole, pidx[keep] - 1, pidx[keep]) if hole >= 0 else pidx[keep]
        ft, xt = eng.batch_fetch_trace(b, len(sel))
        assert 1 <= nfev[b] <= maxfun
        for k in range(int(nfev[b])):
            codes, m = npo.draws(seed, b, base + k + 1, pk, w1, w2)      # numbered by position in the pre-action list
            margin = min(margin, m)
            ref = npo.energy(psi0, (pk, pa, pb, pp), xt[k], ham, codes)
            assert abs(ft[k] - ref) <= E_TOL, ("env-step", b, k, ft[k], ref)
        codes, m = npo.draws(seed, b, base + maxfun + 1, kind, w1, w2)
        margin = min(margin, m)
        ref = npo.energy(psi0, (kind, q0, q1, pidx), xb, ham, codes)
        assert abs(f[b] - ref) <= E_TOL, ("final", b, f[b], ref)
    assert margin > MARGIN
    eng.batch_set_trace(False)
    eng.close()


# ---- 3. the streaming path ---------------------------------------------------------------------------------------------------

def test_streaming_energies_and_env_step(tq):
    """n = 14, batch of 2: k_s_compile draws from the tables; two energy runs, then one env-step whose final evaluation
    (the full list at counter + maxfun + 1, at the parameters it returns) is checked."""
    n, seed, maxfun = 14, 555, 12
    w1, w2 = npo.TABLES["distinct"]
    rng = np.random.default_rng(14)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 12, rng)
    circuits = []
    for b in range(2):
        g = list(tie_free_gates(n, 6, rng))
        g[4] = g[4].astype(np.float32).astype(np.float64)
        circuits.append((with_noise_gates(*g[:4]), g[4]))
    eng = _engine(tq, n, psi0, ham, seed, w1, w2)
    _load(tq, eng, circuits)
    margin = _check_energy_runs(tq, eng, psi0, ham, circuits, seed, w1, w2, (0.0, 0.0), 2)
    eng.batch_set_new_gate([-1, -1])
    eng.batch_run_env_step(1.0, 1e-4, maxfun)
    x, f, nfev = eng.batch_fetch()
    off = 0
    for b, (g, th) in enumerate(circuits):
        xb = x[off:off + th.size]
        off += th.size
        codes, m = npo.draws(seed, b, 2 + maxfun + 1, g[0], w1, w2)
        margin = min(margin, m)
        assert abs(f[b] - npo.energy(psi0, g, xb, ham, codes)) <= E_TOL and 1 <= nfev[b] <= maxfun
    assert margin > MARGIN
    eng.close()


# ---- 4. mode 1 and the quantum-jump runs: the table's channel through the Kraus machinery ---------------------------------------

def test_mode1_equals_the_explicit_kraus_set_and_the_oracle(tq):
    n, seed = 3, 1
    w1, w2 = npo.TABLES["gaps"]
    rng = np.random.default_rng(33)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 12, rng)
    scale = max(1.0, float(np.abs(ham[2]).sum()))
    circuits = _noisy_circuits(n, 3, 14, rng)
    K1, K2 = tq.channels.pauli_channel(w1), tq.channels.pauli_channel(w2)
    want = [dk.circuit_energy(psi0, *g, th, npo.kraus(w1), npo.kraus(w2), ham) for g, th in circuits]
    tab = _engine(tq, n, psi0, ham, seed, w1, w2, p=(0.3, 0.3))
    ovr = _engine(tq, n, psi0, ham, seed, None, None, p=(0.3, 0.3))
    ovr.set_noise_kraus(K1, K2)
    got = {}
    for name, eng in (("table", tab), ("override", ovr)):
        eng.set_noise_mode(1)
        serial = []
        for g, th in circuits:
            eng.set_circuit(tq.Circuit(*g, th.size))
            serial.append(eng.energy(th))
        eng.set_dm_batched(-1)
        _load(tq, eng, circuits)
        eng.batch_run_energy()
        got[name] = (np.array(serial), eng.batch_fetch(want_x=False)[1])
    for k in (0, 1):
        assert np.abs(got["table"][k] - got["override"][k]).max() <= 1e-12
        assert np.abs(got["table"][k] - np.array(want)).max() <= E_TOL
    # one batched gradient against central differences of the oracle: every angle enters as a + b cos + c sin with
    # |b|, |c| <= sum |c_k|, so the difference quotient is off by at most h^2 / 6 of that; rounding adds ~1e-16 / h
    tab.set_dm_grad(True)
    g, th = circuits[0]
    tab.set_circuit(tq.Circuit(*g, th.size))
    e, grad = tab.energy_grad(th)
    h = 1e-4
    ref = np.zeros(th.size)
    for j in range(th.size):
        d = np.zeros(th.size)
        d[j] = h
        ref[j] = (dk.circuit_energy(psi0, *g, th + d, npo.kraus(w1), npo.kraus(w2), ham)
                  - dk.circuit_energy(psi0, *g, th - d, npo.kraus(w1), npo.kraus(w2), ham)) / (2 * h)
    assert abs(e - want[0]) <= E_TOL and np.abs(grad - ref).max() <= h * h * scale, (grad, ref)
    # a Kraus override on a slot wins over the table of that slot
    tab.set_dm_grad(False)
    tab.set_noise_kraus(tq.channels.amplitude_damping(0.3), None)
    ref = dk.circuit_energy(psi0, *g, th, tq.channels.amplitude_damping(0.3), npo.kraus(w2), ham)
    assert abs(tab.energy(th) - ref) <= E_TOL
    tab.close(), ovr.close()


def test_quantum_jumps_of_a_slot_left_to_its_table(tq):
    n, seed, T = 3, 88, 4
    w1, w2 = npo.TABLES["distinct"]
    rng = np.random.default_rng(44)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 12, rng)
    circuits = _noisy_circuits(n, 4, 14, rng)
    ch = tq.channels
    cases = [((ch.amplitude_damping(0.2), None), (None, w2), (ch.amplitude_damping(0.2), ch.pauli_channel(w2))),
             ((None, ch.tensor(ch.amplitude_damping(0.1), ch.dephasing(0.3))), (w1, None),
              (ch.pauli_channel(w1), ch.tensor(ch.amplitude_damping(0.1), ch.dephasing(0.3))))]
    for override, tables, explicit in cases:
        et = []
        for K, w in ((override, tables), (explicit, (None, None))):
            eng = _engine(tq, n, psi0, ham, seed, w[0], w[1], p=(0.3, 0.3))
            eng.set_noise_kraus(*K)
            eng.set_kraus_traj(T)
            _load(tq, eng, circuits)
            eng.batch_run_energy()
            et.append(eng.batch_fetch_traj())
            eng.close()
        assert et[0].shape == (4, T) and np.abs(et[0] - et[1]).max() <= 1e-12
        assert np.ptp(et[0], axis=1).max() > 1e-6      # (the trajectories differ: jumps happened)


# ---- 5. statistics -----------------------------------------------------------------------------------------------------------

def test_sampler_mean_against_the_exact_channel(tq):
    """16 384 streams of one batch: their mean within 4 standard errors of the mode 1 value of the same table - after
    asserting that this value lies at least 10 standard errors from the noiseless energy and from the depolarising channel
    of the same totals (tests/test_noise_pauli_cpu.py checks the same gap on the CPU oracles)."""
    c = npo.stat_case()
    n, N = c["n"], npo.N_SAMPLES
    kind, q0, q1, pidx = c["gates"]
    P, G = c["theta"].size, kind.size
    e_tab, e_dep, e_clean = npo.stat_exact_values(c)
    eng = _engine(tq, n, c["psi0"], c["ham"], c["seed"], c["w1"], c["w2"])
    eng.batch_load_flat(np.arange(N + 1) * G, np.tile(kind, N), np.tile(q0, N), np.tile(q1, N), np.tile(pidx, N),
                        np.arange(N + 1) * P, np.tile(c["theta"], N))
    eng.batch_run_energy()
    f = eng.batch_fetch(want_x=False)[1]
    eng.set_noise_mode(1)
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, P))
    exact = eng.energy(c["theta"])
    sem = f.std(ddof=1) / np.sqrt(N)
    print(f"mean {f.mean():.6f} exact {exact:.6f} (oracle {e_tab:.6f}) sem {sem:.2e}; depolarising {e_dep:.6f} noiseless {e_clean:.6f}")
    assert abs(exact - e_tab) <= E_TOL
    assert abs(exact - e_clean) >= 10 * sem and abs(exact - e_dep) >= 10 * sem
    assert abs(f.mean() - exact) <= 4 * sem
    eng.close()


# ---- 6. lifecycle ------------------------------------------------------------------------------------------------------------

def _refused(tq, code, call):
    with pytest.raises(tq.VQEError, match=f"error {code}:"):
        call()


def test_install_run_remove_and_invalid_inputs(tq):
    n, seed = 4, 17
    w1, w2 = npo.TABLES["distinct"]
    rng = np.random.default_rng(3)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 20, rng)
    circuits = _noisy_circuits(n, 4, 20, rng)
    plain = _engine(tq, n, psi0, ham, seed, None, None)
    used = _engine(tq, n, psi0, ham, seed, w1, w2)
    assert plain.noise_pauli_info() == {"w1": False, "w2": False}
    for eng in (plain, used):
        _load(tq, eng, circuits)
    used.batch_run_energy()
    used.set_noise_pauli(None, None)
    assert used.noise_pauli_info() == {"w1": False, "w2": False}

    def both():
        out = []
        for eng in (plain, used):
            eng.batch_run_energy()
            out.append(eng.batch_fetch(want_x=False)[1])
        return out

    for p in ((0.25, 0.5), (0.0, 0.0)):                      # depolarising, then noiseless: the same bits
        for eng in (plain, used):
            eng.set_noise(p[0], p[1], seed)
        a, b = both()
        assert np.array_equal(a, b)
    # invalid tables: VQE_EINVAL, and the next run has the bits of the handle that was never asked
    for eng in (plain, used):
        eng.set_noise(0.25, 0.5, seed)
    bad1 = [[np.nan, 0.1, 0.1], [-0.1, 0.1, 0.1], [1.5, 0.0, 0.0], [0.5, 0.5, 1e-9]]
    for w in bad1:
        _refused(tq, EINVAL, lambda: used.set_noise_pauli(w, None))
    bad2 = np.full(15, 0.07)
    _refused(tq, EINVAL, lambda: used.set_noise_pauli(None, bad2))
    _refused(tq, EINVAL, lambda: used.set_noise_pauli(w1, bad2))      # one bad table: neither is installed
    with pytest.raises(ValueError):
        used.set_noise_pauli([0.1, 0.1], None)
    assert used.noise_pauli_info() == {"w1": False, "w2": False}
    a, b = both()
    assert np.array_equal(a, b)
    # a later set_noise does not remove a table, and neither call moves the other's setting
    used.set_noise_pauli(w1, w2)
    used.set_noise(0.25, 0.5, seed)
    assert used.noise_pauli_info() == {"w1": True, "w2": True}
    used.batch_run_energy()
    f = used.batch_fetch(want_x=False)[1]
    for b, (g, th) in enumerate(circuits):
        assert abs(f[b] - npo.energy(psi0, g, th, ham, npo.draws(seed, b, 0, g[0], w1, w2)[0])) <= E_TOL
    # mode 0 gradients stay refused, as for depolarising noise
    used.set_noise(0.0, 0.0, seed)
    used.set_circuit(tq.Circuit(*circuits[0][0], circuits[0][1].size))
    _refused(tq, ESTATE, lambda: used.energy_grad(circuits[0][1]))
    plain.close(), used.close()


def test_term_shards_serve_and_amplitude_shards_refuse(tq):
    n, seed = 4, 5
    w1, w2 = npo.TABLES["gaps"]
    rng = np.random.default_rng(8)
    psi0, ham = random_state(n, rng), random_hamiltonian(n, 20, rng)
    circuits = _noisy_circuits(n, 4, 20, rng)
    total = np.zeros(4)
    for rank in range(2):                                    # the draw does not depend on the shard
        eng = _engine(tq, n, psi0, ham, seed, w1, w2)
        eng.set_term_shard(rank, 2)
        _load(tq, eng, circuits)
        eng.batch_run_energy()
        total += eng.batch_fetch(want_x=False)[1]
        eng.close()
    for b, (g, th) in enumerate(circuits):
        assert abs(total[b] - npo.energy(psi0, g, th, ham, npo.draws(seed, b, 0, g[0], w1, w2)[0])) <= E_TOL
    eng = tq.VQEEngine(14)
    eng.set_amplitude_shard(0, 2)
    _refused(tq, ESTATE, lambda: eng.set_noise_pauli(w1, w2))
    assert eng.noise_pauli_info() == {"w1": False, "w2": False}
    eng.set_amplitude_shard(0, 1)
    eng.set_noise_pauli(w1, None)
    _refused(tq, ESTATE, lambda: eng.set_amplitude_shard(0, 2))
    eng.close()


# ---- 7. VecCircuitEnv --------------------------------------------------------------------------------------------------------

def test_vec_env_noise_pauli(tmp_path):
    """The smallest shipped noisy configuration (H2O, 8 qubits) with dephasing-biased tables: the native and the Python
    host loop agree step by step as in tests/test_env_gpu.py, the tables are in force, noise_channel = "exact" runs, and
    a slot takes a table or a Kraus set, not both."""
    import torch
    import tensorrl_qas_amd as tq
    from helpers import make_data_root, reference_config
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent_noise import CircuitEnv
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv as CleanEnv
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    ch = tq.channels
    conf = reference_config("TensorRL_fixed/H2O8q_TNbond2_noise", make_data_root(str(tmp_path / "dmrg-to-qc")))
    conf["non_local_opt"]["global_iters"] = 60
    dev = torch.device("cuda:0")
    w1 = np.array([0.002, 0.002, 0.05])
    w2 = ch.pauli_weights(ch.tensor(ch.dephasing(0.08), ch.dephasing(0.08))) + 0.001
    B = 8
    vn = VecCircuitEnv(CircuitEnv, conf, dev, B, seed=4, native=True, noise_pauli=(w1, w2))
    vp = VecCircuitEnv(CircuitEnv, conf, dev, B, seed=4, native=False, noise_pauli=(w1, w2))
    assert vn.native and not vp.native
    assert vn.engine.noise_pauli_info() == vp.engine.noise_pauli_info() == {"w1": True, "w2": True}
    assert torch.equal(vn.reset(), vp.reset())
    for v in (vn, vp):      # reset() of the Python loop evaluates B energies, the native one none: align the counters
        v.engine.set_noise(CircuitEnv.NOISE_P1, CircuitEnv.NOISE_P2, 4)
    table = vp.envs[0]._actions_table
    rng = np.random.default_rng(17)
    for t in range(5):
        ill = vp.illegal_actions()
        assert vn.illegal_actions() == ill
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
            assert (vn.envs[b].energy, vn.envs[b].error, vn.envs[b].nfev) == (vp.envs[b].energy, vp.envs[b].error, vp.envs[b].nfev)
    assert vn.engine.noise_pauli_info() == {"w1": True, "w2": True}
    ve = VecCircuitEnv(CircuitEnv, conf, dev, 2, seed=4, noise_channel="exact", noise_pauli=(w1, w2))
    ve.reset()
    _, r, _ = ve.step([table[0], table[1]])
    assert ve.engine.noise_mode_info()["mode"] == 1 and bool(torch.isfinite(r).all())
    with pytest.raises(ValueError):
        VecCircuitEnv(CircuitEnv, conf, dev, 2, noise_channel="exact", noise_kraus=(ch.dephasing(0.1), None), noise_pauli=(w1, None))
    with pytest.raises(ValueError):
        VecCircuitEnv(CircuitEnv, conf, dev, 2, noise_pauli=(w1,))
    clean = reference_config("TensorRL_fixed/H2O8q_TNbond2", make_data_root(str(tmp_path / "dmrg-to-qc")))
    with pytest.raises(ValueError):
        VecCircuitEnv(CleanEnv, clean, dev, 2, noise_pauli=(w1, w2))
