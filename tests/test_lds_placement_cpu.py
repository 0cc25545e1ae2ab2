"""CPU: where the device COBYLA of the LDS-resident kernels keeps its arrays (vqe_cobyla_placement - the host-only entry
over cobyla_placement of csrc/vqe_device.h, the function StagedCobyla::init itself calls).  Swept over every compiled
size, every parameter count up to 256 and a few gate / group counts: the invariants the kernel relies on, that every
class occurs, and the list of class boundaries that tests/test_lds_placement_gpu.py runs on both sides of."""
import pytest

import lds_cases as lc

LDS_PER_CU = 160 * 1024
RESIDENT_BUDGET = LDS_PER_CU // 8          # VQE_RESIDENT_BUDGET: the workgroup still fits eight times into a CU
ONE_WAVE_MAX = 9                           # VQE_ONE_WAVE_MAX
SETTINGS = [(0, 1), (0, 40), (64, 8), (400, 8), (400, 200), (1000, 30)]      # (ops beyond the parameters, X-mask groups)


@pytest.fixture(scope="module")
def place():
    import tensorrl_qas_amd as tq
    return tq.cobyla_placement


def _sizes(P, extra_ops):
    mp = lc.round4(P)
    ops = lc.round4(P + extra_ops)
    return ops, min(ops, lc.round4((2 * P + 2) // 3)), mp          # two thirds of the rotations are RX / RY


def _state_bytes(n):
    return 16 << n


def _base_bytes(n, ops, pair, mp, ng):
    """lds_bytes_base, restated from the carve-up's comment in vqe_device.h (struct Lds), for the resident invariant"""
    ng = max(ng, 1)
    b = _state_bytes(n)
    b += 16 * (ops + pair + 2) + 32 * (pair + 2) if n >= 10 else 16 * ops
    b += 16 * mp + 16 * ng + (48 * ng if n >= 10 else 0)
    return b + 128 + 128 + 128 + 32 + 64 + ((2 * ops + 15) & ~15)


@pytest.mark.parametrize("n", lc.SIZES)
def test_invariants_of_every_launch(place, n):
    seen = set()
    for extra, ng in SETTINGS:
        for P in range(1, 257):
            ops, pair, mp = _sizes(P, extra)
            for wide in ((False, True) if n >= lc.WIDE_MIN and mp > 64 else (False,)):
                # a batch whose largest circuit has mp parameters; this circuit has P (and, in a second query, a small one)
                for nvar in {P, min(P, 20), min(P, 40)}:
                    r = place(n, ops, pair, mp, ng, nvar, wide)
                    c = r["class"]
                    seen.add(c)
                    assert c in lc.CLASSES and r["pad"] in (8, 16) and r["words"] > 0
                    if c == "staged":
                        assert r["words"] * 8 <= _state_bytes(n)
                    if c == "resident":
                        assert n <= ONE_WAVE_MAX and r["resident_bytes"] >= r["words"] * 8
                        assert _base_bytes(n, ops, pair, mp, ng) + r["resident_bytes"] + 16 <= RESIDENT_BUDGET
                    else:
                        assert r["resident_bytes"] == 0          # the region exists for the whole batch or not at all
                    if c == "block":
                        assert n >= 10 and nvar > 64 and wide
                    if c == "rows":
                        assert n <= ONE_WAVE_MAX and wide and nvar > 32 and r["pad"] == 16 and r["tile_bytes"] > 0
                    # the tile: only on one-wave sizes in wide launches (which exist from WIDE_MIN qubits and only for
                    # batches with more than 64 parameters)
                    assert (r["tile_bytes"] > 0) == (wide and n <= ONE_WAVE_MAX)
                    assert r["split"] == (nvar <= 32 and c not in ("block", "rows"))
                    # the scratch slice vqe_batch_load reserves per circuit: scratch_doubles(P, 16) + 1 doubles,
                    # = 2 nv^2 + 12 nv + 19 + 1 with nv = P rounded up to 16 (csrc/vqe_api.hip: load_batch)
                    nv16 = (nvar + 15) // 16 * 16
                    assert r["words"] <= 2 * nv16 * nv16 + 12 * nv16 + 20
                    if r["accepted"]:
                        assert r["lds_bytes"] <= LDS_PER_CU
                        assert r["lds_bytes"] >= _base_bytes(n, ops, pair, mp, ng) + r["resident_bytes"] + r["tile_bytes"]
                    else:
                        assert r["lds_bytes"] > LDS_PER_CU or (n >= 10 and ops > (1 << n))
    expect = {"global"}
    expect |= {"resident"} if n <= ONE_WAVE_MAX else {"staged", "block"}
    expect |= {"rows"} if lc.WIDE_MIN <= n <= ONE_WAVE_MAX else set()
    expect |= {"staged"} if 7 <= n <= ONE_WAVE_MAX else set()      # 2 KiB of state hold the arrays of 8 variables
    assert seen == expect, (n, seen, expect)


def test_every_class_occurs(place):
    seen = set()
    for n in lc.SIZES:
        for P in range(1, 257):
            ops, pair, mp = _sizes(P, 400)
            seen.add(place(n, ops, pair, mp, 8, P, n >= lc.WIDE_MIN and mp > 64)["class"])
    assert seen == set(lc.CLASSES)


def _runs(place, n, extra=0, ng=8):
    def classify(P):
        ops, pair, mp = _sizes(P, extra)
        return place(n, ops, pair, mp, ng, P, n >= lc.WIDE_MIN and mp > 64)["class"]
    return lc.class_runs(classify, range(1, 257))


@pytest.mark.parametrize("n", lc.SIZES)
def test_boundary_list(place, n):
    """Single-circuit batches of P rotations and nothing else: the class as P grows, and where it changes.  The
    staged -> global switch of the register path does not depend on the gate or group count (the state region is
    16 << n bytes whatever else the workgroup holds): 24 | 25 at 10 qubits, 40 | 41 at 11, 56 | 57 at 12, none at 13
    (64 variables still fit; from 65 the workgroup-wide context takes over at every n >= 10)."""
    runs = _runs(place, n)
    classes = [r[2] for r in runs]
    edges = lc.boundaries(runs)
    if n < lc.WIDE_MIN:
        assert classes == ["resident", "global"]
    elif n <= ONE_WAVE_MAX:
        assert classes == ["resident", "global", "rows"] and edges[1][:3:2] == (64, 65)
    elif n < 13:
        assert classes == ["staged", "global", "block"] and edges[1][:3:2] == (64, 65)
        assert edges[0][:3:2] == {10: (24, 25), 11: (40, 41), 12: (56, 57)}[n]
        for extra, ng in SETTINGS:
            assert lc.boundaries(_runs(place, n, extra, ng))[0] == edges[0]
    else:
        assert classes == ["staged", "block"] and edges[0][:3:2] == (64, 65)
    # the resident region goes when the workgroup would no longer fit eight times into a CU: earlier with more gates
    # and with more groups, never later
    if n <= ONE_WAVE_MAX:
        last = edges[0][0]
        for extra, ng in SETTINGS:
            r = _runs(place, n, extra, ng)
            assert r[0][2] in ("resident", "staged", "global")
            last_here = r[0][1] if r[0][2] == "resident" else 0
            assert last_here <= last
        # no staged class at all where the state region cannot hold the arrays of even one variable
        no_region = {_runs(place, n, 1000, 30)[0][2]}
        assert no_region == ({"global"} if n <= 6 else {"staged"})
    # lane pairs up to 32 variables, a lane per row beyond, at every size
    for P, want in ((32, True), (33, False)):
        ops, pair, mp = _sizes(P, 0)
        assert place(n, ops, pair, mp, 8, P, False)["split"] is want


def test_small_circuit_in_a_wide_batch(place):
    """One-wave sizes: a 40-parameter circuit next to a 70-parameter one runs the rows context (padding 16), and the
    same circuit alone the plain one-lane-per-row context (padding 8); with 20 parameters lane pairs in both."""
    for n in range(lc.WIDE_MIN, ONE_WAVE_MAX + 1):
        mixed = place(n, 72, 48, 72, 8, 40, True)
        alone = place(n, 40, 28, 40, 8, 40, False)
        assert (mixed["class"], mixed["pad"]) == ("rows", 16) and (alone["class"], alone["pad"]) == ("global", 8)
        assert place(n, 72, 48, 72, 8, 20, True)["split"] and place(n, 72, 48, 72, 8, 20, True)["class"] != "rows"


def test_refusals(place):
    for bad in ((5, 72, 48, 72, 8, 70, 1), (8, 64, 40, 64, 8, 40, 1),      # no launch runs the WIDE variant there
                (0, 4, 4, 4, 1, 1, 0), (14, 4, 4, 4, 1, 1, 0), (4, 4, 8, 4, 1, 1, 0), (4, 4, 4, 4, 1, 5, 0), (4, 4, 4, 4, 1, 0, 0)):
        with pytest.raises(ValueError):
            place(*bad)


def test_compared_cobyla_cases_hang_on_no_marginal_decision():
    """lds_cases.walk_is_decided (CPU only) and the seed walk of cobyla_case: three angles on one qubit over-parametrise
    the state (two real degrees of freedom) and the base seed's walk parts under rounding-size errors inside the compared
    prefix - the case is replaced; ten angles on eight qubits are kept; the chosen case passes the criterion for the
    run that is compared (clean or noisy) and is the same at every call."""
    from helpers import with_noise_gates
    g, th = lc.cobyla_circuit(1, 3, 301)
    assert not lc.walk_is_decided(1, g, th, lc.default_maxfun(3))
    g, th = lc.cobyla_circuit(8, 10, 308)
    assert lc.walk_is_decided(8, g, th, lc.default_maxfun(10))
    assert all((a == b).all() for a, b in zip(lc.cobyla_case(8, 10, 308)[0], g))
    for n, P, seed, noisy in ((1, 3, 301, False), (3, 25, 9325, False), (5, 10, 305, True)):
        g, th = lc.cobyla_case(n, P, seed, noisy)
        seen = with_noise_gates(*g) if noisy else g
        assert lc.walk_is_decided(n, seen, th, lc.default_maxfun(P), (lc.NOISE_SEED, 0, lc.P1, lc.P2) if noisy else None)
        g2, th2 = lc.cobyla_case(n, P, seed, noisy)
        assert (th == th2).all() and all((a == b).all() for a, b in zip(g, g2))
