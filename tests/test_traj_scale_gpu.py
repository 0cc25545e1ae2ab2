"""GPU: the quantum-jump trajectory paths at occupancy, at 16 - 20 qubits and past 4 GiB (tests/traj_scale_cases.py).

1. The LDS-resident path (csrc/vqe_qjump.h, n <= 13), every geometry of sc.LDS_SIZES, with B T >= 2 G + 3 work items on
   the G workgroups of the persistent grid: every workgroup runs at least two items on one LDS image (state, op list,
   (cos, sin) table, reduction scratch, the gate records staged in the state region), circuits of three lengths.
   Selected items against the oracle, the first T' = G // B trajectories bit for bit against a run in which every
   workgroup runs one item, the mean, and the repeat.  The device COBYLA with a grid in its second round at n = 9, 12.
2. The streaming path (csrc/vqe_stream_qjump.h) at 16, 18 and 20 qubits, per trajectory against the oracle.
3. The streaming path with B T = 16 388 resident states of 256 KiB in ONE chunk: the last four begin past 4 GiB
   (tests/test_scale_cases_cpu.py proves the crossing), stream_evaluate runs on a virtual batch of 16 388 streams.  The
   same bits in chunks of 1000 and with max_resident = -1.

Not in scope: the clamp of a chunk to 65 535 states (the y extent of a grid) needs 16 GiB resident at the smallest
streaming size, beyond the scale suite's memory budget per case.

Reference: tests/qj_oracle.py.  Tolerances are the project's: every per-trajectory energy 1e-10 max(1, sum |c_k|),
amplitudes 1e-12; "the same bits" is np.array_equal on the float64 arrays.  The margin precondition (every draw at least
1e-9 from a boundary of its cumulative distribution) is asserted on the oracle alone, on exactly the items compared, ahead
of the comparison.  Per-item jump counts cannot be fetched (kraus_traj_info gives their total over all B T items), so the
jump total is held to the repeat and to the other chunkings, not to the oracle.  Every test prints n, B, T, G, the items
per workgroup, the worst deviation from the oracle, the items compared bit for bit, the bytes held, the wall time of
the device runs and the CPU seconds of the oracle.

Recorded on an MI355X (256 CUs, T = 2732 on the LDS path; worst deviation from the oracle / items bit for bit / oracle s):
  n = 5   G = 4096   2.00 items per workgroup   7.8e-16   4095   0.01      n = 10  G = 2048   4.00   3.3e-16   2046   0.05
  n = 8   G = 4096   2.00                       4.3e-16   4095   0.02      n = 12  G = 512   16.01   4.8e-16    510   0.21
  n = 9   G = 3840   2.13                       6.7e-16   3840   0.03      n = 13  G = 256   32.02   5.1e-16    255   0.49
  the prefix property of (b) held at every size; the device runs of a size take 0.02 s at most.
  COBYLA  n = 9  T = 4096 G = 4096 nfev (10, 12) 2.9e-17, oracle 4 s;  n = 12 T = 1366 G = 512 nfev (12, 10) 1.0e-17, oracle 38 s
          (one oracle mean over all T per circuit: the last evaluation was the result's both times).
  streaming  n = 16: 1.5e-16, amplitudes 2.4e-17;  n = 18: 2.1e-16 and 1.1e-16;  n = 20: 1.3e-16, oracle 4 s.
  one chunk of 16 388 states: 4 456 448 000 bytes held, 34 streams 1.7e-16, 2 x 16 388 items bit for bit, three runs 0.09 s,
          oracle 1.4 s; max_resident = -1 held the whole batch (307 GB free)."""
import time

import numpy as np
import pytest

import qj_cases as qc
import qj_oracle as qo
import scale_cases as sc
import traj_scale_cases as tsc

pytestmark = pytest.mark.gpu
TOL = 1e-10
A_TOL = 1e-12


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _free():
    import torch
    return int(torch.cuda.mem_get_info()[0])


def _scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


def _engine(tq, n, psi0, ham, K1, K2, T, seed, resident=None):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(tsc.P1, tsc.P2, seed)
    eng.set_noise_kraus(K1, K2)
    eng.set_kraus_traj(T)
    if resident is not None:
        eng.set_stream_kraus_traj(resident)
    return eng


def _load(tq, eng, circuits):
    eng.batch_load([tq.Circuit(c[0], c[1], c[2], c[3], c[4].size) for c in circuits], [c[4] for c in circuits])


def _energy_run(eng):
    """-> per-trajectory energies, f, kraus_traj_info, wall seconds"""
    t0 = time.perf_counter()
    eng.batch_run_energy()
    f = eng.batch_fetch(want_x=False)[1].copy()
    et = eng.batch_fetch_traj().copy()
    dt = time.perf_counter() - t0
    return et, f, eng.kraus_traj_info(), dt


def _report(label, n, B, T, G, worst, bitwise, held, wall, oracle_s, more=""):
    print(f"{label}: n={n} B={B} T={T} G={G} items per workgroup={B * T / max(G, 1):.2f} worst deviation={worst:.2e} "
          f"items bit for bit={bitwise} bytes held={held} wall s={wall:.2f} oracle CPU s={oracle_s:.2f}{more}")


# ---- 1. the LDS-resident path: every geometry with several items per workgroup ---------------------------------------
@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_lds_items_per_workgroup(tq, n):
    """(b) rests on a property read from the kernels, not from the header's contract: the draw of (b, e, t, g) does not
    depend on T - key = noise_key(seed, b, eval_id), tsel = (t + 1) << 44 in k_qj_traj - and nothing else in an item
    does, so the first T' trajectories of a run of T are those of a run of T'."""
    psi0, ham, _ = tsc.lds_case(n)
    K1, K2 = qc.combo(tsc.COMBO)
    seed, scale = tsc.LDS_SEED, _scale(ham)
    free0 = _free()
    eng = _engine(tq, n, psi0, ham, K1, K2, 1, seed)
    cus = int(eng.device_info()["cu_count"])
    circuits = tsc.lds_batch(n, cus)[2]
    B, T = len(circuits), tsc.lds_T(cus)
    assert T <= tsc.T_MAX
    eng.set_kraus_traj(T)
    _load(tq, eng, circuits)
    et, f, info, wall = _energy_run(eng)
    held = free0 - _free()
    G = int(info["workgroups"])
    assert et.shape == (B, T) and info["n_traj"] == T and info["evaluations"] == 1
    assert G < B * T and B * T >= 2 * G + 3, (G, B, T)                     # every workgroup ran at least two items

    # (a) the oracle on selected items
    items = tsc.selected_items(n, B, T, G)
    assert set(tsc.pinned_items(B, T, G)) <= set(items)
    t0 = time.process_time()
    want, margin, _ = tsc.oracle_items(psi0, ham, circuits, K1, K2, seed, 0, T, items)
    oracle_s = time.process_time() - t0
    assert margin >= qc.MARGIN, margin                                     # on the oracle alone; no item is left out
    got = np.array([et[w // T, w % T] for w in items])
    dev = np.abs(got - want)
    print(f"n={n}: {len(items)} items against the oracle, margin {margin:.2e}, worst |dE_t| {dev.max():.2e} at item {items[int(dev.argmax())]}")
    assert dev.max() <= TOL * scale, [(w, w // T, w % T, w % G, w // G, d) for w, d in zip(items, dev) if d > TOL * scale][:8]

    # (c) the mean, summed in t order
    for b in range(B):
        assert f[b] == tsc.t_ordered_mean(et[b]), b
    assert info["jumps"] > 0

    # (d) the same evaluation again
    eng.set_noise(tsc.P1, tsc.P2, seed)
    et2, f2, info2, dt = _energy_run(eng)
    wall += dt
    assert np.array_equal(et2, et) and np.array_equal(f2, f) and info2["jumps"] == info["jumps"] and info2["workgroups"] == G
    eng.close()

    # (b) every item of the first T' trajectories, as the first (and only) item of its workgroup
    Ts = G // B
    assert 1 <= Ts < T
    one = _engine(tq, n, psi0, ham, K1, K2, Ts, seed)
    _load(tq, one, circuits)
    et1, _, info1, dt = _energy_run(one)
    wall += dt
    assert info1["workgroups"] == B * Ts <= G, (info1, G)
    later = sum(1 for b in range(B) for t in range(Ts) if b * T + t >= G)
    same = np.array_equal(et[:, :Ts], et1)
    if not same:
        bad = np.argwhere(et[:, :Ts] != et1)
        print(f"n={n}: {len(bad)} of {B * Ts} items differ from their single-item run, the first at (b, t) = {bad[0].tolist()}")
    assert same
    one.close()
    _report(f"trajectories at occupancy ({len(items)} items against the oracle, {later} of the bitwise items in later rounds)",
            n, B, T, G, float(dev.max()), B * Ts, held, wall, oracle_s)


@pytest.mark.parametrize("n", tsc.COBYLA_SIZES)
def test_device_cobyla_at_occupancy(tq, n):
    """The two circuits of test_device_cobyla_and_env_step with so many trajectories that the grid is in its second
    round, and a rhoend at which the two optimisers stop at different evaluations: the items of the circuit that has
    stopped are skipped inside the item loop while its neighbours run.  As there: some evaluation k <= nfev reproduces
    f at the returned x, the oracle's mean over all T trajectories."""
    psi0, ham, _ = qc.parity_case(n)
    circuits = tsc.cobyla_circuits(n)
    K1, K2 = qc.combo(tsc.COMBO)
    B, scale = len(circuits), _scale(ham)
    seed, maxfun, rhoend = tsc.COBYLA_SEED[n], tsc.COBYLA_MAXFUN[n], tsc.COBYLA_RHOEND
    free0 = _free()
    eng = _engine(tq, n, psi0, ham, K1, K2, tsc.T_MAX, seed)
    _load(tq, eng, circuits)
    _, _, info, wall = _energy_run(eng)                                   # the grid of a saturated launch
    T = tsc.cobyla_T(n, B, int(info["workgroups"]))
    eng.set_kraus_traj(T)
    eng.set_noise(tsc.P1, tsc.P2, seed)                                   # the evaluation counter back to 0
    t0 = time.perf_counter()
    eng.batch_run_minimize(1.0, rhoend, maxfun)
    x, f, nfev = eng.batch_fetch()
    wall += time.perf_counter() - t0
    held = free0 - _free()
    info = eng.kraus_traj_info()
    G = int(info["workgroups"])
    assert B * T > G and info["n_traj"] == T, (B, T, G)
    assert np.all((nfev >= 1) & (nfev <= maxfun))
    assert nfev[0] != nfev[1], nfev                                       # the precondition: one circuit idles while the other runs
    worst, off = 0.0, 0
    t0 = time.process_time()
    for b, c in enumerate(circuits):
        xb = x[off:off + c[4].size]
        off += c[4].size
        d = {}
        for k in tsc.evaluation_order(int(nfev[b])):      # every k = 1 .. nfev, the likely ones first, until one fits
            d[k] = abs(f[b] - qo.run(psi0, c[0], c[1], c[2], c[3], xb, K1, K2, ham, seed, b, k, T)["mean"])
            if d[k] <= TOL * scale:
                break
        best = min(d, key=d.get)
        print(f"n={n} minimise circuit {b}: nfev={nfev[b]} f={f[b]:.10f} best k={best} |df|={d[best]:.2e} ({len(d)} evaluations of the oracle)")
        assert d[best] <= TOL * scale, (b, d)
        worst = max(worst, d[best])
    oracle_s = time.process_time() - t0
    eng.close()
    _report(f"device COBYLA at occupancy maxfun={maxfun} rhoend={rhoend} nfev={nfev.tolist()}", n, B, T, G, worst, 0, held, wall, oracle_s)


# ---- 2. the streaming path at 16, 18 and 20 qubits --------------------------------------------------------------------
@pytest.mark.parametrize("n,name", [(n, name) for n in tsc.STREAM_SIZES for name in tsc.stream_combos(n)])
def test_stream_per_trajectory_parity(tq, n, name):
    psi0, ham, circuits = tsc.stream_case(n)
    K1, K2 = qc.combo(name)
    B, T, seed, scale = len(circuits), tsc.STREAM_T, tsc.STREAM_SEED, _scale(ham)
    t0 = time.process_time()
    runs = qc.oracle_runs(psi0, ham, circuits, K1, K2, seed, 1, T)[0]
    oracle_s = time.process_time() - t0
    assert min(r["margin"] for r in runs) >= qc.MARGIN
    want = np.array([r["energies"] for r in runs])
    free0 = _free()
    eng = _engine(tq, n, psi0, ham, K1, K2, T, seed, resident=-1)
    assert not eng.device_info()["lds_path"]
    _load(tq, eng, circuits)
    et, f, info, wall = _energy_run(eng)
    held = free0 - _free()
    sinfo = eng.stream_kraus_traj_info()
    dev = float(np.abs(et - want).max())
    print(f"n={n} {name}: max |dE_t| = {dev:.2e}, jumps {info['jumps']} (oracle {sum(r['jumps'] for r in runs)}), stream info {sinfo}")
    assert et.shape == (B, T) and dev <= TOL * scale, (et, want)
    for b in range(B):
        assert f[b] == tsc.t_ordered_mean(et[b])
        assert abs(f[b] - runs[b]["mean"]) <= TOL * scale
    assert info["n_traj"] == T and info["evaluations"] == 1 and info["jumps"] == sum(r["jumps"] for r in runs)
    assert sinfo["resident"] == B * T == 4 and sinfo["chunks"] == 1
    assert sinfo["rounds"] == max(tsc.noise_gates(c) for c in circuits)
    more = ""
    if n == 16:      # the state of trajectory 0 at the counter (stream 0, evaluation 1)
        c = circuits[0]
        eng.set_circuit(tq.Circuit(c[0], c[1], c[2], c[3], c[4].size))
        psi = eng.get_state(c[4])
        t0 = time.process_time()
        ref = qo.run(psi0, c[0], c[1], c[2], c[3], c[4], K1, K2, ham, seed, 0, 1, 1)
        oracle_s += time.process_time() - t0
        assert ref["margin"] >= qc.MARGIN
        adev = float(np.abs(psi - ref["states"][0]).max())
        more = f" state max |d amp|={adev:.2e}"
        assert adev <= A_TOL and abs(np.linalg.norm(psi) - 1.0) <= A_TOL
    eng.close()
    _report(f"streaming trajectories {name}", n, B, T, int(info["workgroups"]), dev, 0, held, wall, oracle_s, more)


# ---- 3. one chunk past the 4 GiB line -----------------------------------------------------------------------------------
def test_stream_chunk_past_4gib(tq):
    case, n, B, T = "stream_traj", tsc.BIG_N, tsc.BIG_B, tsc.BIG_T
    need = sc.require_memory(case)
    psi0, ham, circuits, order = tsc.big_case()
    K1, K2 = qc.combo(tsc.COMBO)
    total, seed, scale = B * T, tsc.BIG_SEED, _scale(ham)
    items = tsc.big_items()
    t0 = time.process_time()
    want, margin, _ = tsc.oracle_items(psi0, ham, circuits, K1, K2, seed, 0, T, items)
    oracle_s = time.process_time() - t0
    assert margin >= qc.MARGIN, margin

    def run(resident):
        free0 = _free()
        eng = _engine(tq, n, psi0, ham, K1, K2, T, seed, resident=resident)
        _load(tq, eng, circuits)
        et, f, info, dt = _energy_run(eng)
        held = free0 - _free()
        sinfo = eng.stream_kraus_traj_info()
        eng.close()
        return et, f, info, sinfo, held, dt

    # A: everything resident in one chunk
    free_a = _free()
    et, f, info, sinfo, held, wall = run(total)
    assert sinfo["resident"] == total and sinfo["chunks"] == 1, sinfo
    assert et.shape == (B, T)
    got = np.array([et[w // T, w % T] for w in items])
    dev = np.abs(got - want)
    print(f"{case}: {len(items)} streams against the oracle, margin {margin:.2e}, worst |dE_t| {dev.max():.2e} at stream {items[int(dev.argmax())]}")
    assert dev.max() <= TOL * scale, [(w, d) for w, d in zip(items, dev) if d > TOL * scale][:8]
    for b in range(B):
        assert f[b] == tsc.t_ordered_mean(et[b])
    assert sinfo["rounds"] == tsc.BIG_GATES and info["jumps"] > 0

    # B: chunks of 1000, the last ragged
    et_b, f_b, info_b, sinfo_b, _, dt = run(tsc.BIG_CHUNK)
    wall += dt
    assert sinfo_b["resident"] == tsc.BIG_CHUNK and sinfo_b["chunks"] == 17, sinfo_b
    assert np.array_equal(et_b, et) and np.array_equal(f_b, f) and info_b["jumps"] == info["jumps"]

    # C: as many as a quarter of the free memory holds
    per_state = (sc.AMP_BYTES << n) + (((1 << n) // 2 // 2048) * 16 + 32) * 8      # sq_eval's rule (csrc/vqe_api.hip)
    free_c = _free()
    et_c, f_c, info_c, sinfo_c, _, dt = run(-1)
    wall += dt
    R = int(sinfo_c["resident"])
    if (free_c // 4) // per_state >= total:
        branch = "the whole batch fits a quarter of the free memory"
        assert R == min(total, tsc.GRID_Y), sinfo_c
    else:
        branch = "a quarter of the free memory holds a part"
        assert 1 <= R < total, sinfo_c
    assert sinfo_c["chunks"] == -(-total // R), sinfo_c
    assert np.array_equal(et_c, et) and np.array_equal(f_c, f) and info_c["jumps"] == info["jumps"]
    print(f"{case}: max_resident = -1 with {free_c} bytes free ({free_a} before run A): {branch}, resident {R}, chunks {sinfo_c['chunks']}")
    _report(f"{case} ({len(items)} streams against the oracle; runs B and C: all {total} items and f)", n, B, T, int(info["workgroups"]),
            float(dev.max()), 2 * total, held, wall, oracle_s, f" (state-sized buffers {need})")
