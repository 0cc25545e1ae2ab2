"""Paired env-step launches (k_lds_minimize_pair: two environments per workgroup, their two COBYLA updates on two
wavefronts at once) against the unpaired launch on the SAME handle and inputs: energies, x, raw x and nfev equal bit for
bit, and vqe_last_env_pairing says that the paired kernel really ran.  The unpaired path is the yardstick; it is pinned
to the oracle by the other GPU tests.

Shapes: 10 and 12 qubits, 8-16 gates, maxfun <= 60, batches of 1 (a lone environment), 2, 5 (an odd tail) and 9.  The
placement cases at 10 qubits need more rotations than that (a half of the state region holds 1024 doubles there): their
parameter counts are read from vqe_cobyla_placement, not typed in."""
import numpy as np
import pytest

import lds_cases as lc

MAXFUN = 60
MODES = ("batch_run_minimize", "batch_run_env_step")


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _random_batch(tq, n, B, seed):
    rng = np.random.default_rng(seed)
    cs, ths = [], []
    while len(cs) < B:
        c, th = tq.circuits.random_circuit(n, int(rng.integers(8, 17)), rng, p_cnot=0.25)
        if th.size >= 5:      # (the launcher pairs from five parameters per circuit on average)
            cs.append(c), ths.append(th)
    return cs, ths


def _run(eng, mode):
    getattr(eng, mode)(1.0, 1e-4, MAXFUN)
    x, f, nfev = eng.batch_fetch()
    return (f.copy(), x.copy(), eng.batch_fetch_xopt().copy(), nfev.copy()), eng.last_env_pairing()


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _on_vs_off(eng, cs, ths, mode, new_gate=None):
    """-> the paired outputs, after: off == on == on again, and the query's account of both launches"""
    B = len(cs)
    eng.batch_load(cs, ths)
    eng.batch_set_new_gate(new_gate)
    eng.set_env_pairing(False)
    ref, info = _run(eng, mode)
    assert info["paired"] is False and info["pairs"] == 0 and info["singles"] == 0, info
    eng.set_env_pairing(True)
    got, info = _run(eng, mode)
    assert info["paired"] is True and 2 * info["pairs"] + info["singles"] == B, info
    assert info["pairs"] == B // 2, info
    again, info2 = _run(eng, mode)
    assert info2 == info
    assert _same(ref, got), (mode, [np.flatnonzero(u != v) for u, v in zip(ref, got)])
    assert _same(got, again)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 2, 5, 9])
@pytest.mark.parametrize("n", [10, 12])
def test_paired_equals_unpaired(tq, n, B, mode):
    eng = lc.engine(tq, n)
    cs, ths = _random_batch(tq, n, B, 4200 + 10 * n + B)
    new_gate = None
    if mode == "batch_run_env_step":      # the action: the last gate of every circuit
        new_gate = np.array([c.kind.size - 1 for c in cs], np.int32)
    f, _, _, nfev = _on_vs_off(eng, cs, ths, mode, new_gate)
    assert np.all(np.isfinite(f)) and np.all(nfev >= 1) and np.all(nfev <= MAXFUN)
    eng.close()


def _mixed_batch(tq, n):
    """no variables | new gate a CNOT | new gate a rotation (the parameter hole) | one variable, stops at rhoend early |
    a partner that runs to maxfun"""
    C = tq.Circuit
    rng = np.random.default_rng(77 + n)
    no_var = C([0, 0, 0], [0, 1, 2], [1, 2, 3], [-1, -1, -1], 0)
    long_a, th_a = tq.circuits.random_circuit(n, 15, rng, p_cnot=0.2)
    cn = C(np.append(long_a.kind, 0), np.append(long_a.q0, 1), np.append(long_a.q1, 4), np.append(long_a.pidx, -1), th_a.size)
    long_b, th_b = tq.circuits.random_circuit(n, 15, rng, p_cnot=0.2)
    Pb = th_b.size
    rot = C(np.append(long_b.kind, 2), np.append(long_b.q0, 3), np.append(long_b.q1, -1), np.append(long_b.pidx, Pb), Pb + 1)
    one = C([2, 0], [5, 5], [-1, 6], [0, -1], 1)
    long_c, th_c = tq.circuits.random_circuit(n, 16, rng, p_cnot=0.2)
    # hole-only: a single rotation that is the new gate - nothing is left to optimise
    hole_only = C([0, 3], [2, 7], [3, -1], [-1, 0], 1)
    cs = [no_var, cn, rot, one, long_c, hole_only]
    ths = [np.zeros(0), th_a, np.append(th_b, 0.37), np.array([0.4]), th_c, np.array([-1.1])]
    new_gate = np.array([-1, cn.kind.size - 1, rot.kind.size - 1, -1, -1, 1], np.int32)
    return cs, ths, new_gate


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [10, 12])
def test_mixed_phases_in_one_batch(tq, n, mode):
    eng = lc.engine(tq, n)
    cs, ths, new_gate = _mixed_batch(tq, n)
    f, x, xr, nfev = _on_vs_off(eng, cs, ths, mode, new_gate if mode == "batch_run_env_step" else None)
    assert nfev[0] == 1                          # no variables: a single evaluation
    assert 1 < nfev[3] < nfev[4] == MAXFUN       # the one-variable circuit stops at rhoend, its neighbour at maxfun
    if mode == "batch_run_env_step":
        assert nfev[5] == 1                      # only the hole: nothing to optimise
        assert xr[ths[0].size + ths[1].size + ths[2].size - 1] == 0.37      # the hole keeps the action's angle
    eng.close()


def _placement_counts(tq, n):
    """Largest P whose arrays fit a half of the state region, largest P that is staged at all, smallest that is not"""
    half = (16 << n) // 2
    q = {P: tq.cobyla_placement(n, 64, 64, 64, 8, P, False) for P in range(1, 65)}
    fits_half = max(P for P, v in q.items() if v["class"] == "staged" and v["words"] * 8 <= half)
    staged = max(P for P, v in q.items() if v["class"] == "staged")
    assert fits_half < staged < 64 and q[staged + 1]["class"] == "global"
    assert q[fits_half + 1]["words"] * 8 > half
    return fits_half, staged, staged + 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["both_fit_a_half", "one_needs_the_whole_region", "one_is_not_staged"])
def test_placements_at_10_qubits(tq, which, mode):
    n = 10
    fits_half, staged, not_staged = _placement_counts(tq, n)
    Pa = fits_half
    Pb = {"both_fit_a_half": fits_half - 1, "one_needs_the_whole_region": fits_half + 1, "one_is_not_staged": not_staged}[which]
    eng = lc.engine(tq, n)
    pairs = [lc.cobyla_circuit(n, P, 5100 + P) for P in (Pa, Pb)]
    cs = [tq.Circuit(*g, th.size) for g, th in pairs]
    ths = [th for _, th in pairs]
    eng.batch_load(cs, ths)
    want = {"both_fit_a_half": "staged", "one_needs_the_whole_region": "staged", "one_is_not_staged": "global"}[which]
    qa, qb = eng.batch_cobyla_placement(0), eng.batch_cobyla_placement(1)
    half = (16 << n) // 2
    assert qa["class"] == "staged" and qa["words"] * 8 <= half
    assert qb["class"] == want and (qb["words"] * 8 <= half) == (which == "both_fit_a_half")
    _, _, _, nfev = _on_vs_off(eng, cs, ths, mode)
    assert np.all(nfev == MAXFUN)      # past the initial simplex: the update itself ran
    assert max(Pa, Pb) + 2 <= MAXFUN
    eng.close()


@pytest.mark.gpu
def test_trace_and_noise_launch_unpaired(tq):
    n = 10
    eng = lc.engine(tq, n)
    cs, ths = _random_batch(tq, n, 4, 99)
    eng.batch_load(cs, ths)
    eng.batch_run_minimize(1.0, 1e-4, 20)
    assert eng.last_env_pairing()["paired"]
    eng.batch_set_trace(True)
    eng.batch_run_minimize(1.0, 1e-4, 20)
    assert not eng.last_env_pairing()["paired"]
    eng.batch_set_trace(False)
    eng.batch_run_minimize(1.0, 1e-4, 20)
    assert eng.last_env_pairing()["paired"]
    eng.set_noise(0.01, 0.02, 5)
    eng.batch_run_minimize(1.0, 1e-4, 20)
    assert not eng.last_env_pairing()["paired"]
    eng.set_noise(0.0, 0.0, 5)
    eng.batch_run_minimize(1.0, 1e-4, 20)
    assert eng.last_env_pairing()["paired"]
    # fewer than five parameters per circuit on average: the launcher's rule leaves the batch unpaired
    few = [tq.Circuit([1, 0, 2], [0, 0, 3], [-1, 1, -1], [0, -1, 1], 2)] * 4
    eng.batch_load(few, [np.array([0.3, -0.2])] * 4)
    eng.batch_run_minimize(1.0, 1e-4, 20)
    assert not eng.last_env_pairing()["paired"]
    eng.close()


# ---- CPU: the LDS layout of the paired launch -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 11, 12, 13])
@pytest.mark.parametrize("sizes", [(8, 4, 4, 1), (64, 36, 47, 91), (16, 16, 16, 7), (203, 140, 64, 30)])
def test_pair_lds_plan(n, sizes):
    """The second environment's regions lie above everything of the single layout, do not overlap, are 16-byte aligned,
    and the state region is [0, 16 << n)."""
    import tensorrl_qas_amd as tq
    from tensorrl_qas_amd.engine import pair_lds_plan
    max_ops, max_pair, max_params, n_groups = sizes
    p = pair_lds_plan(n, max_ops, max_pair, max_params, n_groups)
    assert p["state_bytes"] == 16 << n
    single = tq.cobyla_placement(n, max_ops, max_pair, max_params, n_groups, 1, False)["lds_bytes"]
    assert p["single_bytes"] == single
    length = {"sched": 16 * (max_ops + max_pair + 2), "lay": 32 * (max_pair + 2), "cs": 16 * max_params, "xm": 4 * 32,
              "zm": 4 * 32, "meta": 4 * 8, "sb": 4 * 16, "sidx": 2 * max_ops, "rec": 2 * 64}
    spans = sorted((p[k], p[k] + length[k], k) for k in length)
    assert spans[0][0] >= single >= p["state_bytes"]
    for (lo, hi, k), (lo2, _, k2) in zip(spans, spans[1:]):
        assert hi <= lo2, (k, k2)
    assert all(lo % 16 == 0 for lo, _, _ in spans)
    assert spans[-1][1] <= p["bytes"] and p["bytes"] % 16 == 0
