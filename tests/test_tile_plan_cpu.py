"""CPU: the planner model (tests/tile_plan_model.py) certifies the case table of the streaming-path planner tests
(tests/stream_cases.py): every case reaches the branch of k_t_plan_ops / k_t_plan_energy (csrc/vqe_tile.h) that its
name promises, and the table as a whole reaches every branch of the checklist below - a fixed condition, not a
measurement.  The model's own invariants are checked on random inputs, its constants against the header.  No GPU: the
values of the same cases are checked against the oracle by tests/test_stream_planner_gpu.py."""
import re

import numpy as np
import pytest

import stream_cases as sc
import tile_plan_model as tm
from stream_cases import RX, RY, RYY

CIRCUITS = sc.circuit_cases()
HAMS = sc.hamiltonian_cases()


def _summary(n, gates, ham, _cache={}):
    key = (n, tuple(gates), tuple(int(v) for v in ham[0]), tuple(int(v) for v in ham[1]), tuple(float(v) for v in ham[2]))
    if key not in _cache:
        _cache[key] = tm.summarize(n, gates, ham)
    return _cache[key]


def test_constants_match_the_header():
    """A retuned tile size must fail here, loudly, before anyone trusts a certificate of the model."""
    assert tm.parse_constants() == tm.model_constants()
    assert tm.kTileK == 3 and tm.kETileFree == tm.kETileBits - tm.kETileLow
    def has(path, *tokens):      # the tokens in this order, whatever the spacing between them
        return re.search(r"\s*".join(re.escape(t) for t in tokens), open(path).read()) is not None
    assert has(tm.TILE_HEADER, "constexpr", "int", "kTileK", "=", "kTileBits", "-", "8", ";")
    assert has(tm.TILE_HEADER, "constexpr", "int", "kETileFree", "=", "kETileBits", "-", "kETileLow", ";")
    stream = tm.TILE_HEADER.replace("vqe_tile.h", "vqe_stream.h")
    assert has(stream, "(", "n_groups", "+", "kETileFree", "-", "1", ")", "/", "kETileFree", "+", "1", "<=", "kMaxEnergyPasses")
    assert has(stream, "n_terms", "<=", str(tm.kMaxTiledTerms))
    # 217 groups: the last count the tiled kernels take
    assert tm.stream_tiled(217, 217) and not tm.stream_tiled(218, 218)


# ---- what every case's name promises ----------------------------------------------------------------------------------
def _dep_chunks(s):
    return [c for c in s["chunks"] if c["dependent"]]


def _flip_promise(kind, code):
    def check(s):
        assert s["passes"] == 1 and len(s["chunks"]) == 1
        c = s["chunks"][0]
        assert c["slots"] == 3 and c["dependent"] == [(kind, code)]      # the dependent op sits in the chunk of its slots
    return check


def _counts(s):
    return [c["count"] for c in s["chunks"]]


def _p_code3_twice(s):
    assert len(s["chunks"]) == 1 and s["chunks"][0]["slots"] == 2 and s["chunks"][0]["dependent"] == [(RX, 3), (RY, 3)]


def _p_xor3(s):
    c = s["chunks"][0]
    assert c["dependent"] == [(RY, 7)] and c["pair_ops"] == 4 and c["ended"] == "fourth"


def _p_rz(counts):
    def check(s):
        assert _counts(s) == counts and all(c["pair_ops"] == 0 and c["fillers"] == 3 for c in s["chunks"])
        assert all(c["ended"] == "cap" for c in s["chunks"][:-1]) and counts[0] == tm.kChunkOps
    return check


def _p_pair3_rz4(s):
    assert _counts(s) == [6, 1]
    a, b = s["chunks"]
    assert (a["pair_ops"], a["fillers"], a["ended"]) == (3, 0, "cap") and (b["pair_ops"], b["fillers"]) == (0, 3)


def _p_pair4(s):
    assert _counts(s) == [3, 1]
    a, b = s["chunks"]
    assert a["ended"] == "fourth" and a["fillers"] == 0 and (b["pair_ops"], b["fillers"]) == (1, 2)


def _p_pair2(s):
    assert _counts(s) == [3] and (s["chunks"][0]["pair_ops"], s["chunks"][0]["fillers"]) == (2, 1)


def _p_low(s):
    # masks in e_0..e_2 never extend the pass basis, yet they take chunk slots
    assert s["passes"] == 1 and s["last_pass_room"] == tm.kTileBits - tm.kTileLow
    assert all(c["low_pair"] and c["slots"] >= 2 for c in s["chunks"])


def _p_full_basis(s):
    assert s["passes"] == 1 and s["last_pass_room"] == 0 and s["n_ops"] == 16


def _p_passes(lo, exact=False):
    def check(s):
        assert s["passes"] == lo if exact else s["passes"] >= lo
    return check


def _p_no_ops(s):
    assert s["n_ops"] == 0 and s["passes"] == 1 and s["chunks"] == []


def _p_one_qubit(s):
    assert s["n_ops"] == 300 and s["passes"] == 1 and s["last_pass_room"] == tm.kTileBits - tm.kTileLow - 1


def _p_last_full(s):
    assert s["last_pass_room"] == 0 and s["fused_groups"] == 0 and s["pair_groups"] >= 3


def _p_room_for_all(s):
    assert s["pair_groups"] >= 3 and s["fused_groups"] == s["pair_groups"] and s["energy_passes"] == 1


def _p_su4_slots(s):
    assert s["chunks"][0]["slots"] == 3 and s["chunks"][0]["dependent"] == [(RYY, 1), (RX, 5)]


def _p_su4_dependent(s):
    assert s["chunks"][0]["slots"] == 3 and s["chunks"][0]["dependent"] == [(RX, 5), (RYY, 7)]      # (RXX compiles to an RX op)


def _p_sweep3(kind):
    def check(s):
        assert s["chunks"][0]["dependent"] == [(kind, 3)]      # (the later triples straddle chunk boundaries: own slots there)
    return check


CIRCUIT_PROMISES = {"flip_code3_twice": _p_code3_twice, "flip_xor3_aligned4": _p_xor3, "chunk_rz7": _p_rz([6, 1]),
                    "chunk_rz13": _p_rz([6, 6, 1]), "chunk_pair3_rz4": _p_pair3_rz4, "chunk_pair4": _p_pair4,
                    "chunk_pair2": _p_pair2, "low_qubits": _p_low, "pass_full_basis": _p_full_basis,
                    "pass_two": _p_passes(2, exact=True), "pass_three": _p_passes(3), "pass_three_n16": _p_passes(3),
                    "empty_circuit": _p_no_ops, "cnot40": _p_no_ops, "one_qubit_300": _p_one_qubit,
                    "last_pass_full": _p_last_full, "last_pass_room_for_all": _p_room_for_all,
                    "su4_slots_and_rider": _p_su4_slots, "su4_dependent": _p_su4_dependent}
for _k in (RX, RY, RYY):
    for _c in range(1, 8):
        CIRCUIT_PROMISES["flip_%s_%d" % (sc.KIND_NAME[_k], _c)] = _flip_promise(_k, _c)
    CIRCUIT_PROMISES["sweep3_" + sc.KIND_NAME[_k]] = _p_sweep3(_k)


def _paths(s):
    return [p.split("@")[0] for p in s["group_paths"]]


def _h_empty(s):
    assert s["n_groups"] == 0 and s["energy_passes"] == 1 and s["pass_group_counts"] == [0]


def _h_diag(classes):
    def check(s):
        assert _paths(s) == ["diagonal"] and s["diag_classes"] == classes and s["fused_groups"] == 0      # kept out of the fused pass
    return check


def _h_no_diag(s):
    assert s["diag_classes"] is None and "diagonal" not in _paths(s) and s["n_groups"] == 3


def _h_terms(n_groups):
    def check(s):
        assert _paths(s)[:4] == ["general:1", "general:2:refused-unequal", "general:3+", "general:3+"]
        assert s["pass_group_counts"] == [n_groups]
    return check


def _h_imag(s):
    where = {p.split("@")[1] for p in s["group_paths"] if ":imag" in p}
    assert where == {"fused", "own"}


def _h_half(s):
    got = {p for p in _paths(s) if p.startswith("half")}
    assert got == {"half:%s:%s" % (a, b) for a in ("equal", "opposite") for b in ("q<hb", "q>hb")}


def _h_refused(why):
    def check(s):
        assert any(p.endswith("refused-" + why) for p in _paths(s))
    return check


def _h_many(s):
    assert s["energy_passes"] >= 3 and s["own_passes"] >= 3
    assert {c % 2 for c in s["own_pass_group_counts"]} == {0, 1}      # e_tile_groups takes the groups of a pass two at a time


def _h_217(s):
    assert s["tiled"] and s["n_groups"] == 217 and s["energy_passes"] >= 3


def _h_218(s):
    assert not s["tiled"] and s["n_groups"] == 218


HAM_PROMISES = {"ham_empty": _h_empty, "ham_identity": _h_diag([0]), "ham_diag_one_class": _h_diag([3]),
                "ham_diag_eight_classes": _h_diag(list(range(8))), "ham_no_diagonal": _h_no_diag,
                "ham_terms_1_2_3_odd_groups": _h_terms(5), "ham_terms_even_groups": _h_terms(6),
                "ham_imaginary_fused_and_own": _h_imag, "ham_half_chain": _h_half,
                "ham_half_refused_unequal": _h_refused("unequal"), "ham_half_refused_zero": _h_refused("zero"),
                "ham_half_refused_imaginary": _h_refused("imaginary"), "ham_half_refused_czd0": _h_refused("czd0"),
                "ham_many_passes": _h_many, "ham_217_groups": _h_217, "ham_218_groups": _h_218}


def test_case_names_are_unique_and_promised():
    names = [c[0] for c in CIRCUITS] + [h[0] for h in HAMS]
    assert len(names) == len(set(names))
    assert {c[0] for c in CIRCUITS} == set(CIRCUIT_PROMISES) and {h[0] for h in HAMS} == set(HAM_PROMISES)


@pytest.mark.parametrize("case", CIRCUITS, ids=[c[0] for c in CIRCUITS])
def test_circuit_case_reaches_its_branch(case):
    name, _, n, gates, ham = case
    CIRCUIT_PROMISES[name](_summary(n, gates, ham))


@pytest.mark.parametrize("case", HAMS, ids=[h[0] for h in HAMS])
def test_hamiltonian_case_reaches_its_branch(case):
    """The promise holds behind the empty circuit; the two-pass background is certified to be two passes (its CNOTs
    move the masks, so the paths behind it are whatever the planner then decides - the device has to get them right
    all the same)."""
    name, n, ham, backgrounds = case
    assert backgrounds[0] == "empty"
    HAM_PROMISES[name](_summary(n, [], ham))
    if "two_pass" in backgrounds:
        s = _summary(n, sc.background("two_pass", n), ham)
        assert s["passes"] == 2 and s["n_groups"] == len(set(int(x) for x in ham[0]))


# ---- the aligned sweeps of the gradient's backward kernel (three ops) and of the untiled kernels (four) -----------------
def test_sweep_kernels_reach_their_generic_flip_codes():
    """k_sg_back<3> and k_s_opk<4> cut the op list into aligned groups of K ops from op 0 and have a generic branch for
    an op whose mask is the XOR of several slots of its group.  Certified here, for the circuits the GPU module runs:
    the gradient test (every flip-group circuit behind 0, 1 and 2 extra RZ) reaches code 3 with RX, RY and RYY at
    every one of the three prefixes; the untiled run (the same circuits, no prefix) reaches codes 3 and 7."""
    flip = [c for c in CIRCUITS if c[1] == "flip"]

    def generic(gates, K):
        ops = tm.compile_gates(sc.N, gates)[0]
        return {d for grp in tm.sweep_flip_codes(ops, K) for d in grp if d[1] & (d[1] - 1)}

    for prefix in (0, 1, 2):
        head = [(sc.RZ, q, -1) for q in (sc.A, 2)[:prefix]]
        for kind in (RX, RY, RYY):
            assert (kind, 3) in generic(head + sc.sweep3_circuit(kind), 3), (prefix, kind)
        reached = set().union(*(generic(head + c[3], 3) for c in flip))
        assert {(RX, 3), (RY, 3), (RYY, 3)} <= reached
    reached4 = set().union(*(generic(c[3], 4) for c in flip))
    assert {code for _, code in reached4} >= {3, 7}
    assert (RY, 7) in generic(sc.xor3_aligned4(), 4)
    assert {(RX, 3), (RY, 3), (RYY, 3)} <= reached4


# ---- the checklist ----------------------------------------------------------------------------------------------------
def _required_branches():
    req = {"passes:1", "passes:2", "passes:3+",
           "last:full-none-fused", "last:room-all-fused", "last:some-fused-rest-own",
           "chunk:pair-ops-0", "chunk:pair-ops-1", "chunk:pair-ops-2", "chunk:pair-ops-3", "chunk:cap", "chunk:fourth",
           "fillers:0", "fillers:1", "fillers:2", "fillers:3", "pair-op-in-tile-low",
           "energy-passes:1", "energy-passes:2", "energy-passes:3+",
           "diag:1-class", "diag:8-classes", "diag:none",
           "general:1", "general:2", "general:3+", "imag:fused", "imag:own",
           "fused-pass:odd", "fused-pass:even", "own-pass:odd", "own-pass:even",
           "groups:empty", "groups:217-tiled", "groups:218-untiled"}
    req |= {"dep:%s:%d" % (k, c) for k in ("rx", "ry") for c in range(1, 8)} | {"dep:ryy:3", "dep:ryy:7"}
    req |= {"half:%s:%s" % (a, b) for a in ("equal", "opposite") for b in ("q<hb", "q>hb")}
    req |= {"refused:" + w for w in ("unequal", "zero", "imaginary", "czd0")}
    return req


def branches_of(s):
    """The checklist entries one summary reaches."""
    out = set()
    if not s["tiled"]:
        return {"groups:218-untiled"} if s["n_groups"] == 218 else set()
    out.add("passes:%s" % (s["passes"] if s["passes"] < 3 else "3+"))
    if s["pair_groups"]:
        if s["last_pass_room"] == 0 and s["fused_groups"] == 0:
            out.add("last:full-none-fused")
        elif s["last_pass_room"] > 0 and s["fused_groups"] == s["pair_groups"]:
            out.add("last:room-all-fused")
        elif 0 < s["fused_groups"] < s["pair_groups"]:
            out.add("last:some-fused-rest-own")
    for c in s["chunks"]:
        if c["pair_ops"] <= 3:
            out.add("chunk:pair-ops-%d" % c["pair_ops"])
        if c["ended"] == "cap" and c["count"] == tm.kChunkOps:
            out.add("chunk:cap")
        if c["ended"] == "fourth":
            out.add("chunk:fourth")
        out.add("fillers:%d" % c["fillers"])
        if c["low_pair"]:
            out.add("pair-op-in-tile-low")
        for kind, code in c["dependent"]:
            out.add("dep:%s:%d" % (tm.OP_NAME[kind], code))
    out.add("energy-passes:%s" % (s["energy_passes"] if s["energy_passes"] < 3 else "3+"))
    if s["n_groups"] == 0:
        out.add("groups:empty")
    else:
        if s["diag_classes"] is None:
            out.add("diag:none")
        elif len(s["diag_classes"]) in (1, 8):
            out.add("diag:%s" % ("1-class" if len(s["diag_classes"]) == 1 else "8-classes"))
    if s["n_groups"] == 217:
        out.add("groups:217-tiled")
    for c in s["own_pass_group_counts"]:
        out.add("own-pass:" + ("odd" if c % 2 else "even"))
    if s["fused_groups"]:
        out.add("fused-pass:" + ("odd" if s["fused_groups"] % 2 else "even"))
    for p in s["group_paths"]:
        what, where = p.split("@")
        f = what.split(":")
        if f[0] == "half":
            out.add(what)
        elif f[0] == "general":
            out.add("general:" + f[1])
            if "imag" in f:
                out.add("imag:" + where)
            if f[-1].startswith("refused-"):
                out.add("refused:" + f[-1][len("refused-"):])
    return out


def coverage():
    """branch -> the cases that reach it (circuit cases; Hamiltonian cases behind each of their backgrounds)"""
    cov = {}
    for name, _, n, gates, ham in CIRCUITS:
        for b in branches_of(_summary(n, gates, ham)):
            cov.setdefault(b, []).append(name)
    for name, n, ham, backgrounds in HAMS:
        for bg in backgrounds:
            for b in branches_of(_summary(n, sc.background(bg, n), ham)):
                cov.setdefault(b, []).append("%s/%s" % (name, bg))
    return cov


def test_the_table_reaches_every_branch():
    cov = coverage()
    missing = sorted(_required_branches() - set(cov))
    assert not missing, missing
    for b in sorted(_required_branches()):
        print("%-28s %s" % (b, ", ".join(cov[b][:4]) + (" (+%d)" % (len(cov[b]) - 4) if len(cov[b]) > 4 else "")))


# ---- the model's own invariants ---------------------------------------------------------------------------------------
def _random_gates(n, G, rng):
    out = []
    for _ in range(G):
        u = rng.random()
        a = int(rng.integers(n))
        b = int((a + 1 + rng.integers(n - 1)) % n)
        if u < 0.35:
            out.append((sc.CX, a, b))
        elif u < 0.55:
            out.append((int(rng.choice((sc.RXX, sc.RYY, sc.RZZ))), a, b))
        else:
            out.append((int(rng.choice((RX, RY, sc.RZ))), a, -1))
    return out


def _check_basis(b, low, bits):
    assert b.dim == bits and b.piv == sorted(b.piv) and len(set(b.piv)) == bits
    assert b.v[:low] == [1 << i for i in range(low)]
    for i, (v, p) in enumerate(zip(b.v, b.piv)):
        assert tm.top_bit(v) == p
        assert all(not (w >> p) & 1 for j, w in enumerate(b.v) if j != i)      # fully reduced


@pytest.mark.parametrize("n,G,T,seed", [(14, 0, 0, 0), (14, 12, 9, 1), (14, 60, 40, 2), (14, 200, 120, 3), (16, 90, 60, 4),
                                        (16, 40, 217, 5), (20, 120, 77, 6)])
def test_model_invariants(n, G, T, seed):
    rng = np.random.default_rng(9000 + seed)
    gates = _random_gates(n, G, rng)
    xs = rng.integers(0, 1 << n, T)
    xs[: T // 5] = 0                                    # a diagonal group
    if T > 6:
        xs[T // 2:T // 2 + 3] = xs[T // 2]              # groups of several terms
    ham = (xs.astype(np.uint64), rng.integers(0, 1 << n, T).astype(np.uint64), rng.normal(size=T))
    for fuse in (True, False):
        p = tm.plan(n, gates, ham, fuse)
        if not p["tiled"]:
            assert len(set(xs.tolist())) > 217
            continue
        ops, passes = p["ops"], p["passes"]
        # passes tile the op list; every pair op of a pass has its mask in the pass's span
        assert passes[0]["begin"] == 0 and passes[-1]["end"] == len(ops)
        seen = [0] * len(ops)
        for i, ps in enumerate(passes):
            _check_basis(ps["basis"], tm.kTileLow, tm.kTileBits)
            if i:
                assert ps["begin"] == passes[i - 1]["end"] and tm.op_is_pair(ops[ps["begin"]].kind)
            for o in range(ps["begin"], ps["end"]):
                assert not tm.op_is_pair(ops[o].kind) or ps["basis"].reduce(ops[o].xm) == 0
            at = ps["begin"]
            for c in ps["chunks"]:                      # chunks tile the pass
                assert c["begin"] == at and 1 <= c["count"] <= tm.kChunkOps and c["slots"] + c["fillers"] == tm.kTileK
                for j in range(c["count"]):
                    seen[at + j] += 1
                    if tm.op_is_pair(ops[at + j].kind):
                        x = 0
                        for k in range(tm.kTileK):
                            if (c["flips"][j] >> k) & 1:
                                x ^= c["slot_masks"][k]
                        assert c["flips"][j] and x == ps["basis"].coords(ops[at + j].xm)
                    else:
                        assert c["flips"][j] == 0
                at += c["count"]
            assert at == ps["end"]
        assert seen == [1] * len(ops)
        # every group belongs to exactly one energy pass, and its mask closes inside that pass's tile
        owner = [0] * p["n_groups"]
        assert 1 <= len(p["epasses"]) <= tm.kMaxEnergyPasses
        for k, e in enumerate(p["epasses"]):
            fused = fuse and k == 0
            _check_basis(e["basis"], tm.kTileLow if fused else tm.kETileLow, tm.kETileBits)
            if fused:
                assert e["basis"].v == passes[-1]["basis"].v
            for g in e["groups"]:
                owner[g] += 1
                x = p["pgroups"][g][0]
                assert e["basis"].reduce(x) == 0 and p["groups"][g]["pass"] == k and not (fused and x == 0)
        assert owner == [1] * p["n_groups"]
