"""CPU: the scenarios of tests/handle_cases.py are worth running (no GPU: the oracle and the library's host-only queries).

A handle that answers a step with what it computed for an EARLIER step - a stale buffer, a plan of the previous
generation - passes the GPU test wherever the two steps expect the same value.  So every scenario is held to a condition:
the expected result of each step differs, in max-norm, by more than 1e-6 from the expected result of every earlier step
of the scenario with the same output shape.  Steps that are meant to return the bits of an earlier one (the walk comes
back to its first configuration; a run is repeated behind another kind of run) are declared as such in the scenario, and
the GPU test asserts the equality of their bits instead.  The expected value of an optimiser run is what the host
COBYLA (the library's, bit-exact with scipy) or the numpy restatement of the device L-BFGS finds on the oracle's
objective.  Seeds are chosen for which the condition holds; a discarded seed is printed."""
import numpy as np
import pytest

import handle_cases as hc
from lds_cases import round4


@pytest.mark.parametrize("name", hc.NAMES)
def test_steps_expect_distinct_values(name):
    w = hc.scenario(name)
    d, pair = hc.min_distance(w)
    declared = sum(st.same_as is not None for st in w.steps)
    print(f"{w.name}: {len(w.steps)} steps ({declared} declared to repeat an earlier one), "
          f"smallest distance between expected values {d:.3e} ({pair})")
    assert d > hc.DISTINCT
    assert all(st.fp is not None for st in w.steps), "a step without an expected value"
    # a step declared to repeat an earlier one expects that one's value
    for st in w.steps:
        if st.same_as is not None and st.fp is not None:
            assert np.abs(st.fp - w.steps[st.same_as].fp).max() < 1e-9, st.label


def test_recorded_seeds_are_the_first_that_pass():
    """handle_cases.SEEDS holds every scenario whose seed 0 was discarded - and only those, with the first seed that
    passes (the procedure is first_distinct_seed, which prints what it discards)"""
    print("discarded seeds (scenario: seed in use):", hc.SEEDS or "none")
    for name, seed in hc.SEEDS.items():
        assert seed > 0 and hc.first_distinct_seed(name) == seed, name


def test_noisy_steps_are_replayed_only_at_counter_zero():
    """a fresh handle starts its evaluation counter at 0: a noisy step elsewhere is compared with the oracle's draws only"""
    for n in (6, 10):
        w = hc.scenario(f"S5-n{n}")
        fresh = [st.fresh for st in w.steps]
        assert not all(fresh) and sum(fresh) >= 8, fresh


@pytest.mark.parametrize("n", [4, 10])
def test_s3_changes_placement_class_between_runs(n):
    """vqe_cobyla_placement (host only) for the largest circuit of each of the five batches, with the sizes vqe_batch_load
    derives: consecutive runs on the one handle place the optimiser's arrays differently.  At 10 qubits every run
    changes the class (staged, global, block of the wide launch, global, staged); at 4 qubits there is no wide launch
    (n < 6) and 64 and 70 parameters are both in the global scratch, so there the class changes at the first and the last
    transition and the layout (the doubles the arrays take) at every one."""
    import tensorrl_qas_amd as tq
    ham = hc.inputs(n)[1]
    groups = int(np.unique(ham[0]).size)
    sig = []
    for cs, ths, ng in hc.s3_batches(n):
        ops = [int(np.count_nonzero(c.kind != 0)) for c in cs]
        pair = [int(np.count_nonzero(np.isin(c.kind, (1, 2)))) for c in cs]
        P = max(c.P for c in cs)
        max_ops, max_params = round4(max(max(ops), 1)), round4(max(P, 1))
        max_pair = min(max_ops, round4(max(pair)))
        p = tq.cobyla_placement(n, max_ops, max_pair, max_params, groups, P, n >= 6 and max_params > 64)
        assert p["accepted"], p
        sig.append((p["class"], p["pad"], p["split"], p["words"]))
        assert {0, 1} <= {c.P for c in cs} or len(cs) == 1 or min(c.P for c in cs) == 0
        assert max(len(c.kind) for c in cs) >= 25 or len(cs) < 70
    print(f"n={n}: placement of the largest circuit, batch by batch: {sig}")
    assert all(a != b for a, b in zip(sig, sig[1:])), sig
    cls = [s[0] for s in sig]
    assert cls == (["staged", "global", "block", "global", "staged"] if n == 10 else ["resident", "global", "global", "global", "resident"])


def _n_blocks(n, c, th):
    """vqe_dm_plan (host only): the superoperator blocks the exact channel mode sweeps for this circuit"""
    import ctypes as C
    from tensorrl_qas_amd import _lib
    nb = C.c_int32()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib.c_i32p)
    th = np.ascontiguousarray(th if len(th) else np.zeros(1), np.float64)
    assert _lib.load().vqe_dm_plan(n, len(c.kind), i32(c.kind), i32(c.q0), i32(c.q1), i32(c.pidx), th.ctypes.data_as(_lib.c_f64p),
                                   0.05, 0.2, 0, C.byref(nb), None, None) == 0
    return nb.value


@pytest.mark.parametrize("n", [4, 5])
def test_s6_block_counts_change_with_the_circuit(n):
    """the batch of S6 has circuits of different block counts (one of them 0), and the pre-action batches of its two
    new-gate arrays are different circuits: a plan kept from the first env-step would be wrong for the second"""
    cs, th_a, _, ng1, ng2 = hc.s6_batches(n)
    full = [_n_blocks(n, c, t) for c, t in zip(cs, th_a)]
    pre = [[hc.pre_action(c, t, int(g)) for c, t, g in zip(cs, th_a, ng)] for ng in (ng1, ng2)]
    counts = [[_n_blocks(n, p[0], p[1]) for p in batch] for batch in pre]
    print(f"n={n}: blocks of the full circuits {full}, of the pre-action circuits {counts}")
    assert 0 in full and len(set(full)) >= 3
    differ = [len(a[0].kind) != len(b[0].kind) or any(np.any(u != v) for u, v in zip(a[0][:4], b[0][:4])) for a, b in zip(*pre)]
    assert sum(differ) >= 3, differ
    assert all(len(p[0].kind) < len(c.kind) for p, c, g in zip(pre[0], cs, ng1) if g >= 0)
    assert any(len(c.kind) - len(p[0].kind) == 2 for p, c in zip(pre[0], cs))      # a channel left with its gate


def test_s7_names_its_exemptions():
    """the steps of the streaming scenario that are compared at 1e-12: each carries the line of vqe_stream.h behind it"""
    w = hc.scenario("S7-n14")
    loose = [(st.label, st.loose) for st in w.steps if st.loose]
    for label, why in loose:
        print(f"S7 step {label}: {why}")
    assert {why for _, why in loose} == {hc.LINE_472, hc.LINE_490, hc.LINE_513}
    for name in hc.NAMES:
        if name != "S7-n14":
            assert not any(st.loose for st in hc.scenario(name).steps), name
