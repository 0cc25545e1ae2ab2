"""CPU: the case tables of tests/scale_cases.py - the batch layout puts copies where the occupancy tests need them, the
two comparison helpers bite (one flipped bit, one value off by 2e-10), the distinct circuits of a case differ in length,
and every case of part B reaches past 4 GiB by the library's own size rules.  No GPU."""
import numpy as np
import pytest

import lds_cases as lc
import scale_cases as sc


@pytest.mark.parametrize("grid", [1, 2, 5, 256, 512, 2048])
@pytest.mark.parametrize("K", [3, 4, 5, 6])
def test_tile_order_places_the_copies(K, grid):
    order = sc.tile_order(K, grid, seed=K)
    B = grid + 3
    assert order.size == B and order.min() >= 0 and order.max() < K
    pin = sc.pinned_positions(grid)
    assert {0, 1, grid - 1, grid, grid + 1, B - 1} & set(range(B)) == set(pin)
    assert all(order[p] == 0 for p in pin)
    for i in range(1, B):      # neighbours differ, except where both are pinned copies of circuit 0
        assert order[i] != order[i - 1] or (i in pin and i - 1 in pin), (i, order[i - 1:i + 1])
    assert np.array_equal(order, sc.tile_order(K, grid, seed=K))      # fixed
    if grid >= 256:      # every circuit has copies in both rounds' neighbourhood: a group to compare, and an oracle position
        assert all((order == k).sum() >= 2 for k in range(K))
        assert sorted(sc.last_positions(order, K))[-1] == B - 1


def test_stream_order_with_two_circuits():
    order = sc.stream_order(2, sc.BENCH_B)
    assert order.size == sc.BENCH_B and set(order.tolist()) == {0, 1}
    assert all(order[p] == 0 for p in (0, 1, sc.BENCH_B - 4, sc.BENCH_B - 3, sc.BENCH_B - 2, sc.BENCH_B - 1))
    assert (order == 1).sum() >= 100 and order[2] == 1


def test_copy_comparison_bites_on_one_flipped_bit():
    order = sc.tile_order(4, 256)
    rng = np.random.default_rng(0)
    per = rng.normal(size=(4, 7))
    f = [float(per[k, 0]) for k in order]
    x = [per[k].copy() for k in order]
    assert sc.assert_copies_identical(order, {"f": f, "x": x}) == 4
    victim = int(np.nonzero(order == 2)[0][-1])
    bad = [v.copy() for v in x]
    bad[victim][3] = (bad[victim][3:4].view(np.uint64) ^ np.uint64(1)).view(np.float64)[0]      # the last bit of one word
    assert abs(bad[victim][3] - x[victim][3]) < 1e-15
    with pytest.raises(AssertionError, match="x: circuit 2"):
        sc.assert_copies_identical(order, {"f": f, "x": bad})
    fbad = list(f)
    fbad[victim] = float((np.array([f[victim]]).view(np.uint64) ^ np.uint64(1)).view(np.float64)[0])
    with pytest.raises(AssertionError, match="f: circuit 2"):
        sc.assert_copies_identical(order, {"f": fbad, "x": x})
    # a sign of zero is a bit too
    z = [0.0] * order.size
    z[victim] = -0.0
    with pytest.raises(AssertionError):
        sc.assert_copies_identical(order, {"z": z})


def test_oracle_comparison_bites_at_twice_the_tolerance():
    ref = np.array([-1.25, 0.5, 3.0])
    assert sc.assert_close("e", ref + 0.5e-10, ref, lc.E_TOL) <= lc.E_TOL
    with pytest.raises(AssertionError, match="exceeds"):
        sc.assert_close("e", ref + np.array([0.0, 2e-10, 0.0]), ref, lc.E_TOL)
    with pytest.raises(AssertionError):
        sc.assert_close("e", np.array([np.nan, 0.5, 3.0]), ref, lc.E_TOL)
    with pytest.raises(AssertionError, match="exceeds"):
        sc.assert_close("e", -1.25 + 2e-10, -1.25, lc.E_TOL)


@pytest.mark.parametrize("n", sc.LDS_SIZES + (sc.MANY_N,))
def test_distinct_circuits_differ_in_length(n):
    sets = [sc.many_circuits()] if n == sc.MANY_N else [sc.energy_circuits(n), sc.grad_circuits(n)]
    for circuits in sets:
        assert 4 <= len(circuits) <= 6
        assert len({g[0].size for g, _ in circuits}) == len(circuits)
        assert len({th.size for _, th in circuits}) == len(circuits)
    if n != sc.MANY_N:      # the lengths of the size tests at this n are among them
        assert min(20 + 4 * n, 70) in [g[0].size for g, _ in sc.energy_circuits(n)]
        assert min(12 + 3 * n, 40) in [g[0].size for g, _ in sc.grad_circuits(n)]
        assert sc.small_p(n) == 10 and len(set(sc.MIN_P + (10,))) == 4


@pytest.mark.parametrize("n", sc.WIDE_SIZES)
def test_wide_classes_are_the_placement_functions(n):
    """wide_class against the library's own decision function (host only), with batch sizes of the wide cases' order"""
    import tensorrl_qas_amd as tq
    ng = len(set(lc.inputs(n)[1][0].tolist()))
    for P in set(sc.WIDE_P):
        q = tq.cobyla_placement(n, 100, 68, 68, ng, P, True)
        assert (q["class"], q["pad"]) == sc.wide_class(n, P), (n, P, q)
        if P > 64:      # the arrays of such a circuit live in the global scratch, at scratch_begin[circuit]
            assert q["class"] in ("rows", "block") and q["words"] * 8 > (16 << n) // 2


@pytest.mark.parametrize("case", sc.BIG_CASES)
def test_big_cases_cross_the_line(case):
    """The largest offset a case reaches in each of its state-sized buffers is at least one stride past 2^32 bytes."""
    offs = sc.largest_offsets(case)
    assert offs
    for name, (elem, byte, stride) in offs.items():
        print(f"{case}: {name}: largest slice begins at element {elem} = byte {byte}, {byte - sc.LINE} bytes "
              f"({(byte - sc.LINE) / stride:.1f} strides of {stride} B) past 2^32")
        if name in sc.NOT_CROSSING:
            continue
        assert byte >= sc.LINE + stride, (case, name, byte)
        if case != "dm_grad":      # (its size is set by the levels of one circuit, not by a batch)
            assert byte + stride <= 5 * 2 ** 30      # and no further than it has to
    need = sc.bytes_needed(case)
    print(f"{case}: {need / 2 ** 30:.2f} GiB held")
    assert need <= 10.5 * 2 ** 30


def test_trainable_batch_comes_from_the_placement_rule():
    """B = ceil(2^32 / (8 words)) + 3 with words from vqe_cobyla_placement: the last circuit's scratch begins at least one
    stride past 2^32 bytes, the circuit three places before it does not"""
    words = sc.trainable_words()
    B, stride = sc.trainable_batch(words), sc.scratch_stride(words)
    assert words >= 2 * sc.TRAIN_P ** 2 and words <= stride < words + 17
    print(f"trainable_scratch: words={words} stride={stride} doubles B={B}: last circuit at byte {(B - 1) * stride * 8}")
    assert (B - 1) * stride * 8 >= sc.LINE + stride * 8
    assert (B - 4) * words * 8 < sc.LINE
    circuits = sc.trainable_circuits()
    assert all(th.size == sc.TRAIN_P for _, th in circuits) and len({g[0].size for g, _ in circuits}) == 2
    assert all(abs(int((g[0] == 0).sum()) - sc.TRAIN_CNOTS) <= 10 for g, _ in circuits)


def test_gradient_stack_of_one_circuit_straddles_the_line():
    """Level l of resident slot s lies at ((l + 1) R + s) << 2 n entries: the levels of circuit 0 alone begin below
    2^32 bytes and end above"""
    levels = sc.dm_grad_levels()
    assert sc.DMG_MIN_LEVELS <= levels <= sc.DMG_MAX_LEVELS
    at = [(((l + 1) * sc.DMG_R + 0) << (2 * sc.DM_N)) * sc.AMP_BYTES for l in range(levels + 1)]
    print(f"dm_grad: {levels} levels, rho_0 of circuit 0 at byte {at[0]}, rho_{levels} at byte {at[-1]} "
          f"({at[-1] - sc.LINE} past 2^32)")
    assert at[0] < sc.LINE and at[-1] >= sc.LINE + (sc.AMP_BYTES << (2 * sc.DM_N))
    assert at[-1] + (sc.AMP_BYTES << (2 * sc.DM_N)) * sc.DMG_R == sc.bytes_needed("dm_grad")
    e, g = sc.dm_grad_oracle()
    assert np.abs(g).max() > 1e-3


def test_exact_channel_circuits():
    """Three different circuits whose CNOTs reach the two highest qubits in both orders, no gate across a partition (the
    factorised oracle is exact), and energies that the channels move"""
    import dm_factor_oracle as fo
    three, states, psi0, ham = sc.dm_problem()
    circuits = sc.dm_circuits()
    assert len({c[4].size for c in circuits}) == 3 and len({len(c[0]) for c in circuits}) == 3
    n = sc.DM_N
    for k, (parts, c) in enumerate(zip(three, circuits)):
        assert not fo.crosses(parts, c)
        cnots = {(int(a), int(b)) for kd, a, b in zip(c[0], c[1], c[2]) if kd == 0}
        for q in (n - 1, n - 2):
            assert any(a == q for a, _ in cnots) and any(b == q for _, b in cnots), (k, q, cnots)
        e = sc.dm_oracle_energy(k, c[4])
        clean = fo.energy(n, parts, states[k], c[:4], c[4], ham, *sc.DM_NOISE, noiseless=True)
        assert abs(e - clean) > 1e-6 and abs(e) > 1e4 * lc.E_TOL, (k, e, clean)
    order = sc.tile_order(3, sc.DM_B - 3, 12)
    assert order.size == sc.DM_B and all((order == k).sum() >= 2 for k in range(3))
