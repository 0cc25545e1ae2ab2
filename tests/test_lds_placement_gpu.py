"""GPU: the device COBYLA on BOTH sides of every boundary between the places its arrays can live (an LDS region of their
own, the idle state region, the global scratch with one wave / with the row walks / with the whole workgroup, lane
pairs per row) - at every compiled size.  A staging copy that is off by one word or a budget check off by 16 bytes
corrupts the optimiser's matrices only at these edges.

No parameter count is typed in here except the two the kernel source names itself (32 | 33: lane pairs, 64 | 65: the wide
launch): every other edge is FOUND by asking vqe_batch_cobyla_placement about loaded batches - the kernel's own decision
function - and a boundary that a size does not have is asserted absent by the same query.  On each side: the query
reports the intended class, every traced value is the oracle's energy at the traced point, and the library's host
COBYLA, told the device's values, walks the same points (lds_cases.check_trace; the circuit of each run is the first
of its seeds whose walk hangs on no marginal decision - lds_cases.walk_is_decided, CPU only).  The two resident edges grow the gate
count (rotations that share parameter 0) resp. the X-mask groups of the Hamiltonian until the query flips, so their
circuits are as long as the remaining LDS budget asks for."""
import numpy as np
import pytest

import lds_cases as lc

pytestmark = pytest.mark.gpu

P_SCAN = range(1, 71)
ONE_WAVE_MAX = 9


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _seed(n, P):
    return 9000 + 100 * n + P


def _query(eng, tq, n, P, extra_rz=0, case=None):
    """The placement of a single-circuit batch of P parameters (+ extra_rz ops): of ``case`` if given, else of the
    circuit of the base seed (the class depends on the op and parameter counts alone, which every seed shares)."""
    gates, th = case if case is not None else lc.cobyla_circuit(n, P, _seed(n, P), extra_rz)
    eng.batch_load([tq.Circuit(*gates, P)], [th])
    q = eng.batch_cobyla_placement(0)
    # the handle-free entry, fed what the handle feeds its own, says the same
    sizes = lc.single_circuit_sizes(gates, P)
    free = tq.cobyla_placement(n, *sizes, eng.hamiltonian_layout()["table_groups"], P, n >= lc.WIDE_MIN and sizes[2] > 64)
    assert free == q, (n, P, q, free)
    assert q["accepted"]
    return q


def _run(eng, tq, n, P, want, extra_rz=0, noisy=False):
    gates, th = lc.cobyla_case(n, P, _seed(n, P), noisy, extra_rz)
    q = _query(eng, tq, n, P, extra_rz, (gates, th))
    assert q["class"] == want, (n, P, want, q)
    lc.minimize_and_check(eng, tq, n, gates, th, noisy)
    return q


def _runs(eng, tq, n):
    return lc.class_runs(lambda P: _query(eng, tq, n, P)["class"], P_SCAN)


@pytest.mark.parametrize("n", lc.SIZES)
def test_lds_to_global_edge(tq, n):
    """The largest P whose arrays are in LDS (resident up to 9 qubits, staged from 10) and the smallest in the global
    scratch.  13 qubits have no such edge: 64 variables still fit into the state region."""
    eng = lc.engine(tq, n)
    runs = _runs(eng, tq, n)
    classes = [r[2] for r in runs]
    in_lds = "resident" if n <= ONE_WAVE_MAX else "staged"
    if n == 13:
        assert classes == ["staged", "block"], runs
        eng.close()
        return
    assert classes[:2] == [in_lds, "global"], runs
    last, first = runs[0][1], runs[1][0]
    assert first == last + 1 <= 64
    q0 = _run(eng, tq, n, last, in_lds)
    q1 = _run(eng, tq, n, first, "global")
    if n > ONE_WAVE_MAX:      # staged: the arrays fit into the state region
        assert q0["words"] * 8 <= (16 << n)
    assert q1["resident_bytes"] == 0
    print(f"n={n}: {in_lds} up to P={last}, global from {first}")
    eng.close()


@pytest.mark.parametrize("n", lc.SIZES)
def test_lane_pair_edge(tq, n):
    """32 | 33 variables: two lanes per row | a lane per row - clean on both sides, and noisy (check 4) on the far one."""
    eng = lc.engine(tq, n)
    qs = [_query(eng, tq, n, P) for P in (32, 33)]
    assert [q["split"] for q in qs] == [True, False], qs
    for P, q in zip((32, 33), qs):
        _run(eng, tq, n, P, q["class"])
    eng2 = lc.engine(tq, n)
    gates, th = lc.cobyla_case(n, 33, _seed(n, 33), True)
    lc.minimize_and_check(eng2, tq, n, gates, th, True)
    eng.close(), eng2.close()


@pytest.mark.parametrize("n", [n for n in lc.SIZES if n >= lc.WIDE_MIN])
def test_wide_launch_edge(tq, n):
    """64 | 65 variables: the plain minimiser | the WIDE one (rows context on one wave, workgroup-wide from 10 qubits)"""
    eng = lc.engine(tq, n)
    q64 = _query(eng, tq, n, 64)
    assert q64["class"] in ("global", "staged") and q64["tile_bytes"] == 0 and q64["pad"] == 8
    _run(eng, tq, n, 64, "staged" if n == 13 else "global")
    q65 = _run(eng, tq, n, 65, "rows" if n <= ONE_WAVE_MAX else "block")
    assert (q65["tile_bytes"] > 0) == (n <= ONE_WAVE_MAX)
    eng.close()


def _mixed_query(eng, tq, n, P, big):
    gates, th = lc.cobyla_circuit(n, P, _seed(n, P))
    eng.batch_load([tq.Circuit(*gates, P), tq.Circuit(*big[0], big[1].size)], [th, big[1]])
    return eng.batch_cobyla_placement(0)


@pytest.mark.parametrize("n", [n for n in lc.SIZES if n <= ONE_WAVE_MAX])
def test_staged_edge_of_the_one_wave_sizes(tq, n):
    """Up to 9 qubits the arrays are staged into the state region only in a batch that has no resident region - here:
    next to a 60-parameter circuit - and only while they fit into 16 << n bytes.  Where not even one variable fits
    (up to 6 qubits) the class must not occur."""
    eng = lc.engine(tq, n)
    big = lc.cobyla_circuit(n, 60, _seed(n, 60))
    runs = lc.class_runs(lambda P: _mixed_query(eng, tq, n, P, big)["class"], range(1, 33))
    classes = [r[2] for r in runs]
    if classes == ["global"]:      # even the tighter global layout of ONE variable is larger than the state region
        assert 8 * tq.cobyla_placement(n, 60, 60, 60, 1, 1, False)["words"] > (16 << n)
        assert n <= 6
        eng.close()
        return
    assert classes == ["staged", "global"], runs
    last, first = runs[0][1], runs[1][0]
    maxfun = 60 + 1 + lc.AFTER_SIMPLEX
    for P, want in ((last, "staged"), (first, "global")):
        gates, th = lc.cobyla_case(n, P, _seed(n, P), maxfun=maxfun)
        eng.batch_load([tq.Circuit(*gates, P), tq.Circuit(*big[0], big[1].size)], [th, big[1]])
        assert eng.batch_cobyla_placement(0)["class"] == want
        _, _, _, nfev, tr = lc.traced_minimize(eng, tq, [(gates, th), big], maxfun)
        lc.check_trace(tq, n, gates, th, tr[0][0], tr[0][1], int(nfev[0]), maxfun)
    print(f"n={n}: staged up to P={last} in a batch without a resident region")
    eng.close()


@pytest.mark.parametrize("n", [n for n in lc.SIZES if n <= ONE_WAVE_MAX])
def test_resident_edge_by_gate_count(tq, n):
    """At the largest resident P: more gates (4 at a time - the handle rounds to 4) until the region no longer fits"""
    eng = lc.engine(tq, n)
    P = _runs(eng, tq, n)[0][1]
    extra = 0
    while _query(eng, tq, n, P, extra + 4)["class"] == "resident":
        extra += 4
        assert extra < 4096
    _run(eng, tq, n, P, "resident", extra)
    after = _query(eng, tq, n, P, extra + 4)
    # (9 qubits: the arrays of the 16 variables then fit into the state region; below they go to the global scratch)
    assert after["class"] in ("staged", "global") and after["resident_bytes"] == 0
    _run(eng, tq, n, P, after["class"], extra + 4)
    print(f"n={n} P={P}: resident with {extra} more ops, {after['class']} with {extra + 4}")
    eng.close()


@pytest.mark.parametrize("n", [n for n in lc.SIZES if n <= ONE_WAVE_MAX])
def test_resident_edge_by_group_count(tq, n):
    """At the largest resident P: more X-mask groups in the Hamiltonian until the region no longer fits.  Where all 2^n
    masks together do not use the budget up, the query must still say resident with all of them."""
    psi0, ham = lc.inputs(n)
    eng = lc.engine(tq, n)
    P = _runs(eng, tq, n)[0][1]
    gates, th = lc.cobyla_circuit(n, P, _seed(n, P))
    have = {int(x) for x in ham[0]}
    spare = [x for x in range(1 << n) if x not in have]
    rng = np.random.default_rng(8800 + n)
    coef = 1e-2 * rng.normal(size=len(spare))

    def with_groups(k):
        return (np.concatenate([ham[0], np.array(spare[:k], np.uint64)]), np.concatenate([ham[1], np.zeros(k, np.uint64)]),
                np.concatenate([ham[2], coef[:k]]))

    def cls(k):
        eng.set_hamiltonian(*with_groups(k))
        eng.batch_load([tq.Circuit(*gates, P)], [th])
        return eng.batch_cobyla_placement(0)["class"]

    if cls(len(spare)) == "resident":
        print(f"n={n} P={P}: resident with all {1 << n} X masks - no group edge at this size")
        assert n < ONE_WAVE_MAX
        eng.close()
        return
    lo, hi = 0, len(spare)          # resident with lo more groups, not with hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if cls(mid) == "resident" else (lo, mid)
    maxfun = P + 1 + lc.AFTER_SIMPLEX + 8
    for k in (lo, hi):
        assert (cls(k) == "resident") == (k == lo)
        gk, tk = lc.cobyla_case(n, P, _seed(n, P), maxfun=maxfun, ham=with_groups(k))
        _, _, f, nfev, tr = lc.traced_minimize(eng, tq, [(gk, tk)], maxfun)
        assert (eng.batch_cobyla_placement(0)["class"] == "resident") == (k == lo)
        lc.check_trace(tq, n, gk, tk, tr[0][0], tr[0][1], int(nfev[0]), maxfun, ham=with_groups(k))
    print(f"n={n} P={P}: resident with {lo} more groups, {cls(hi)} with {hi}")
    eng.close()
