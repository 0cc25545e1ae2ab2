"""CPU: the case tables of tests/traj_scale_cases.py - the item-selection helpers name the items they promise, the ``ts``
option of qj_oracle.run returns the rows of the full run, the circuits hold what their docstrings say, T stays within
the ABI's limit for 64 ... 512 CUs, the big chunk ends past 4 GiB within the scale suite's memory budget, and the part of
every checked set that does not depend on the device has no draw within 1e-9 of a boundary under the committed seeds.
No GPU."""
import numpy as np
import pytest

import qj_cases as qc
import qj_oracle as qo
import scale_cases as sc
import traj_scale_cases as tsc

GRIDS = [(3, 2732, 256), (3, 2732, 4096), (3, 2732, 3840), (3, 11, 7), (2, 4096, 4096), (2, 1366, 512), (3, 5, 40), (1, 9, 4)]


@pytest.mark.parametrize("B,T,G", GRIDS)
def test_item_selection(B, T, G):
    total = B * T
    pin = tsc.pinned_items(B, T, G)
    assert set(pin) == {w for w in (0, 1, G - 1, G, G + 1, 2 * G - 1, 2 * G, total - 1) if 0 <= w < total}
    for g in (0, 1, G - 1):
        seq = tsc.workgroup_items(g, B, T, G)
        want = [w for w in range(total) if w % G == g]
        assert seq == want and tsc.workgroup_items(g, B, T, G, 3) == want[:3]
    change = tsc.circuit_change_items(B, T, G)
    assert len(set(change)) == len(change) and len({w % G for w in change}) == len(change)      # one per residue class
    for w in change:
        assert G <= w < total and w // T != (w - G) // T
        assert all(v // T == (v - G) // T for v in range(w % G + G, w, G))                        # ... and the first of its class
    every = [w for w in range(G, total) if w // T != (w - G) // T]
    assert {w % G for w in every} == {w % G for w in change}                                      # no class left out
    capped = tsc.circuit_change_items(B, T, G, 16)
    assert len(capped) == min(16, len(change)) and set(capped) <= set(change)
    if total > G:
        sample = tsc.sampled_items(5, B, T, G)
        assert len(sample) == min(tsc.SAMPLE, total - G) == len(set(sample)) and all(G <= w < total for w in sample)
        assert sample == tsc.sampled_items(5, B, T, G)
    sel = tsc.selected_items(5, B, T, G)
    assert all(0 <= w < total for w in sel) and len(sel) <= 8 + tsc.WG0_CAP + tsc.CHANGE_CAP + tsc.SAMPLE
    assert set(pin) <= set(sel) and set(capped) <= set(sel)


def test_trajectory_counts_fit_the_abi():
    """T <= 4096 for 64 ... 512 CUs, and every workgroup of the largest grid runs two items with three to spare"""
    for cus in (64, 104, 128, 228, 256, 304, 512):
        B, T = tsc.lds_B(cus), tsc.lds_T(cus)
        G = tsc.WG_PER_CU_MAX * cus
        assert T <= tsc.T_MAX and B * T >= 2 * G + 3 > B * (T - 1), (cus, B, T)
        assert B == (3 if cus <= 383 else 5)
        circuits = tsc.lds_batch(5, cus)[2]
        assert len(circuits) == B and all(circuits[b][0].size != circuits[b + 1][0].size for b in range(B - 1))
    assert tsc.lds_T(256) == 2732
    for n in tsc.COBYLA_SIZES:
        for G in (256, 512, 2048, 3840, 4096, 8192):
            T = tsc.cobyla_T(n, 2, G)
            assert tsc.COBYLA_T[n] <= T <= tsc.T_MAX and (2 * T > G or T == tsc.T_MAX)


def test_evaluation_order_lists_every_evaluation_and_suits_the_host_cobyla():
    """On the library's host COBYLA (the device loop's algorithm) with the occupancy test's rhobeg, rhoend and maxfun and
    an objective with a different error in every evaluation: the order holds every k once, and the evaluation that
    produced the result is met after two oracle calls on average."""
    import tensorrl_qas_amd as tq
    asked = []
    for trial in range(40):
        rng = np.random.default_rng(trial)
        P = int(rng.integers(5, 9))
        x0, a = rng.uniform(-np.pi, np.pi, P), rng.normal(size=P)
        opt = tq.HostCobyla(x0, 1.0, tsc.COBYLA_RHOEND, 12)
        xs, fs = [], []
        while (x := opt.ask()) is not None:
            xs.append(x)
            fs.append(float(np.sin(x + a).sum() + (0.3, 5.0)[trial % 2] * rng.normal()))
            opt.tell(fs[-1])
        xr, fr, nfev, _ = opt.result()
        assert nfev == len(xs) >= min(12, P + 1)
        made = [k + 1 for k in range(nfev) if np.array_equal(xs[k], xr) and fs[k] == fr]
        assert made, trial
        order = tsc.evaluation_order(nfev)
        assert sorted(order) == list(range(1, nfev + 1))
        asked.append(1 + min(order.index(k) for k in made))
    print(f"oracle calls until the result's evaluation is met: mean {np.mean(asked):.2f}, most {max(asked)}")
    assert np.mean(asked) <= 2.0


def test_oracle_ts_rows_are_the_full_runs():
    n, T = 5, 16
    psi0, ham, circuits = qc.parity_case(n)
    K1, K2 = qc.combo(tsc.COMBO)
    c = circuits[1]
    full = qo.run(psi0, *c, K1, K2, ham, 77, 1, 2, T)
    ts = [11, 0, 15, 3, 3]
    part = qo.run(psi0, *c, K1, K2, ham, 77, 1, 2, T, ts=ts)
    for key in ("states", "energies", "ks"):
        assert np.array_equal(part[key], full[key][ts]), key
    assert np.array_equal(part["slot_kind"], full["slot_kind"])
    assert part["margin"] >= full["margin"] and part["jumps"] == int(np.count_nonzero(full["ks"][ts]))
    assert part["mean"] == tsc.t_ordered_mean(full["energies"][ts])
    again = qo.run(psi0, *c, K1, K2, ham, 77, 1, 2, T, ts=range(T))
    assert all(np.array_equal(again[k], full[k]) for k in ("states", "energies", "ks")) and again["mean"] == full["mean"]
    assert np.array_equal(qo.run(psi0, *c, K1, K2, ham, 77, 1, 2, 4096, ts=ts)["energies"], full["energies"][ts])      # (no T in a draw)
    with pytest.raises(AssertionError):
        qo.run(psi0, *c, K1, K2, ham, 77, 1, 2, T, ts=[T])
    en, margin, states = tsc.oracle_items(psi0, ham, circuits, K1, K2, 77, 2, T, [T + 11, 3, 2 * T, T])
    assert np.array_equal(en[[0, 3]], full["energies"][[11, 0]]) and np.array_equal(states[T + 11], full["states"][11])
    r0 = qo.run(psi0, *circuits[0], K1, K2, ham, 77, 0, 2, T)
    assert en[1] == r0["energies"][3] and margin >= min(full["margin"], r0["margin"])


@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_lds_circuits(n):
    psi0, ham, circuits = tsc.lds_case(n)
    assert psi0.size == 1 << n and ham[2].size == 14 and len(circuits) == tsc.LDS_B
    assert [c[0].size for c in circuits] == [2 * G for G in tsc.LDS_LENGTHS]
    assert len({c[4].size for c in circuits}) == tsc.LDS_B
    for c in circuits:
        assert set(int(v) for v in c[0]) == set(range(9))               # all nine kinds, both noise gates among them
        assert np.all((c[0][1::2] == 4) | (c[0][1::2] == 5))
    K1, K2 = qc.combo(tsc.COMBO)
    assert len(K1) == 2 and len(K2) == 4 and abs(K1[1][0, 1]) > 0        # a jump that is no Pauli


@pytest.mark.parametrize("n", tsc.COBYLA_SIZES)
def test_cobyla_circuits_are_those_of_the_small_test(n):
    a, b = tsc.cobyla_circuits(n)
    assert a[0].size == b[0].size == 2 * tsc.COBYLA_GATES and not np.array_equal(a[0], b[0])
    rng = np.random.default_rng(8800 + n)
    for c in (a, b):
        assert all(np.array_equal(u, v) for u, v in zip(c, qc.noisy_su4(n, 9, rng)))


@pytest.mark.parametrize("n", tsc.STREAM_SIZES)
def test_stream_circuits(n):
    psi0, ham, circuits = tsc.stream_case(n)
    assert psi0.size == 1 << n and ham[2].size == 14
    assert [c[0].size for c in circuits] == [2 * G for G in tsc.STREAM_LENGTHS]
    for c, G in zip(circuits, tsc.STREAM_LENGTHS):
        assert all(tsc.gate_classes(c[0]).values()) and tsc.noise_gates(c) == G
        assert int(c[3].max()) + 1 == c[4].size
    assert tsc.stream_combos(18) == qc.COMBOS and tsc.stream_combos(16) == tsc.stream_combos(20) == (tsc.COMBO,)


def test_big_chunk_crosses_the_line():
    psi0, ham, circuits, order = tsc.big_case()
    n, B, T = tsc.BIG_N, tsc.BIG_B, tsc.BIG_T
    assert len(circuits) == B == order.size and set(order.tolist()) == {0, 1, 2}
    assert all(c[0].size == 2 * tsc.BIG_GATES and tsc.noise_gates(c) == tsc.BIG_GATES for c in circuits)
    base = qc.parity_case(n)[2]
    for b, k in enumerate(order):
        for u, v in zip(circuits[b][:4], base[k][:4]):
            assert np.array_equal(u, v[:2 * tsc.BIG_GATES])
        assert np.array_equal(circuits[b][4], base[k][4][:circuits[b][4].size])
    last = (B * T - 1) * (sc.AMP_BYTES << n)
    assert last >= sc.LINE and last == sc.largest_offsets("stream_traj")["states"][1]
    assert sc.bytes_needed("stream_traj") <= 10.5 * 2 ** 30 and "stream_traj" in sc.BIG_CASES
    assert B * T < tsc.GRID_Y and -(-B * T // tsc.BIG_CHUNK) == 17 and (B * T) % tsc.BIG_CHUNK != 0
    items = tsc.big_items()
    assert {0, 1, 16383, 16384, 16387} <= set(items) and all(0 <= w < B * T for w in items)
    blocks = {w // T for w in items if w % T == 0} & {w // T for w in items if w % T == T - 1}
    assert len({int(order[b]) for b in blocks}) == 3                      # first and last item of blocks of all three circuits
    assert len(items) <= 5 + 6 + tsc.BIG_SAMPLE


# ---- margins of the device-independent part of every checked set ------------------------------------------------------
@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_lds_margins(n):
    """The pinned items that do not depend on the grid and the seeded samples for grids of 256 x {1, 2, 8, 16}"""
    psi0, ham, circuits = tsc.lds_case(n)
    K1, K2 = qc.combo(tsc.COMBO)
    B, T = tsc.LDS_B, tsc.lds_T(tsc.CPU_CUS)
    items = {0, 1, B * T - 1}
    for wg in tsc.CPU_WG:
        items |= set(tsc.sampled_items(n, B, T, tsc.CPU_CUS * wg))
    _, margin, _ = tsc.oracle_items(psi0, ham, circuits, K1, K2, tsc.LDS_SEED, 0, T, sorted(items))
    print(f"n={n}: {len(items)} items, smallest margin {margin:.2e}")
    assert margin >= qc.MARGIN


@pytest.mark.parametrize("n", tsc.STREAM_SIZES)
def test_stream_margins(n):
    psi0, ham, circuits = tsc.stream_case(n)
    for name in tsc.stream_combos(n):
        K1, K2 = qc.combo(name)
        runs = qc.oracle_runs(psi0, ham, circuits, K1, K2, tsc.STREAM_SEED, 1, tsc.STREAM_T)[0]
        print(f"n={n} {name}: smallest margin {min(r['margin'] for r in runs):.2e}, jumps {sum(r['jumps'] for r in runs)}")
        assert min(r["margin"] for r in runs) >= qc.MARGIN


def test_big_chunk_margins():
    psi0, ham, circuits, _ = tsc.big_case()
    K1, K2 = qc.combo(tsc.COMBO)
    _, margin, _ = tsc.oracle_items(psi0, ham, circuits, K1, K2, tsc.BIG_SEED, 0, tsc.BIG_T, tsc.big_items())
    print(f"big chunk: smallest margin {margin:.2e}")
    assert margin >= qc.MARGIN
