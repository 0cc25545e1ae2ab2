"""CPU: the pre-action circuit of an environment step - the rule (pre_action, csrc/vqe_geo.h) that the streaming path
and the exact channel mode share, and the host halves built on it (csrc/env_step_host.h).  The fused kernel holds a
hand-kept copy of the rule (k_lds_minimize's prologue), which this test cannot see: the GPU env-step tests pin that.

tests/cpp/env_step_check.cpp (g++, no HIP) runs the library's own routines over small gate lists; every expected value -
skip, skip_end, hole, the pre-action gate list, x0, and x / xraw after the optimiser - is computed HERE from the rule
as include/vqe_hip.h states it at vqe_batch_set_new_gate, and compared exactly:

* new_gate < 0: nothing left out, no hole;
* the new gate is left out; if it is a rotation (RX .. RZZ) its parameter is the hole: not a variable, every higher
  parameter index moves down by one, and after the optimiser it keeps its theta0 value;
* the gate behind it is left out with it exactly when it is the channel the noisy ansatz builder attached: a DEPOL1
  behind a one-qubit rotation on the same qubit, a DEPOL2 behind a CNOT on the same (q0, q1) - never behind
  RXX / RYY / RZZ, never when the new gate is the last one;
* x is xraw rounded to float32 in an environment step, xraw itself otherwise.

Cases: every new-gate kind x every follower x the new gate first / in the middle / last but one (the follower is the
circuit's final gate: what an RL action that appends a gate and its channel gives), the new gate last (no follower),
new_gate = -1, and circuits whose other parameters all lie above / all below the hole; 3-6 gates on 3 qubits."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "env_step_check.cpp")

CNOT, RX, RY, RZ, DEPOL1, DEPOL2, RXX, RYY, RZZ = range(9)
ROT1, ROT2 = (RX, RY, RZ), (RXX, RYY, RZZ)
TWO_QUBIT = (CNOT, DEPOL2) + ROT2
FOLLOWERS = ("depol1_same", "depol1_other", "depol2_same", "depol2_swapped", "depol2_other", "rotation")
NQ = 3


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("env_step") / "env_step_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def _gate(kind, q0, q1=None):
    """[kind, q0, q1, pidx] with pidx still open (-1); one-qubit gates carry q1 = -1."""
    return [kind, q0, q1 if kind in TWO_QUBIT else -1, -1]


def _follower(name, new, rng):
    _, q0, q1, _ = new
    others = [q for q in range(NQ) if q not in (q0, q1)]
    if q1 < 0:
        q1 = others.pop()        # a one-qubit new gate: "its pair" is (q0, some other qubit)
    other = others[0]
    return {"depol1_same": _gate(DEPOL1, q0), "depol1_other": _gate(DEPOL1, other),
            "depol2_same": _gate(DEPOL2, q0, q1), "depol2_swapped": _gate(DEPOL2, q1, q0),
            "depol2_other": _gate(DEPOL2, q0, other),
            "rotation": _gate(int(rng.choice(ROT1)), q0)}[name]


def _filler(rng):
    kind = int(rng.integers(0, 9))
    q0, q1 = (int(q) for q in rng.permutation(NQ)[:2])
    return _gate(kind, q0, q1)


def _number_parameters(gates, order):
    """Gives the rotations their parameter indices: the i-th rotation of the list gets order[i]."""
    rots = [g for g in gates if g[0] in ROT1 + ROT2]
    for g, p in zip(rots, order):
        g[3] = int(p)
    return len(rots)


def _make_cases():
    rng = np.random.default_rng(20261017)
    cases = []      # (gates, P, new_gate)

    def add(before, new, after, hole_rank=None, no_new_gate=False):
        gates = [list(g) for g in before + [new] + after]
        n_rot = sum(g[0] in ROT1 + ROT2 for g in gates)
        order = rng.permutation(n_rot)
        if hole_rank is not None:      # the new rotation gets the lowest (0) or the highest (-1) parameter index
            at = sum(g[0] in ROT1 + ROT2 for g in before)
            rest = [p for p in range(n_rot) if p != (0 if hole_rank == 0 else n_rot - 1)]
            order = list(rng.permutation(rest))
            order.insert(at, 0 if hole_rank == 0 else n_rot - 1)
        P = _number_parameters(gates, order)
        assert 3 <= len(gates) <= 6
        cases.append((gates, P, -1 if no_new_gate else len(before)))

    for kind in range(9):
        q0, q1 = (int(q) for q in rng.permutation(NQ)[:2])
        new = _gate(kind, q0, q1)
        for name, position in itertools.product(FOLLOWERS, ("first", "middle", "last_but_one")):
            before = [] if position == "first" else [_filler(rng) for _ in range(int(rng.integers(1, 3)))]
            after = [_follower(name, new, rng)]
            if position == "last_but_one":      # the follower is the final gate: new_gate == G - 2
                before += [_filler(rng) for _ in range(int(rng.integers(0, 3)))]
            else:
                after += [_filler(rng) for _ in range(int(rng.integers(1, 3)))]
            add(before, new, after)
        # the new gate is the last one: no follower
        add([_filler(rng) for _ in range(int(rng.integers(2, 6)))], new, [])
        # no new gate at all, the same kinds of circuit
        add([_filler(rng)], new, [_follower("depol2_same" if kind == CNOT else "depol1_same", new, rng), _filler(rng)],
            no_new_gate=True)
    # every other parameter above the hole / below it (with an attached channel and without)
    for hole_rank, kind in itertools.product((0, -1), (RY, RZZ)):
        rots = [_gate(RX, 0), _gate(RZ, 1), _gate(RYY, 2, 0)]
        new = _gate(kind, 1, 2)
        add(rots[:2], new, [_gate(DEPOL1, 1), rots[2]], hole_rank=hole_rank)
        add(rots[:1], new, rots[1:], hole_rank=hole_rank)
    return cases


def _expected(gates, P, new_gate, theta, xopt):
    """The rule, restated: (skip, skip_end, hole), pre-action gates, x0, xraw."""
    skip, skip_end, hole = -1, 0, -1
    if new_gate >= 0:
        kind, q0, q1, pidx = gates[new_gate]
        skip, skip_end = new_gate, new_gate + 1
        if kind in ROT1 + ROT2:
            hole = pidx
        if new_gate + 1 < len(gates):
            fk, fq0, fq1, _ = gates[new_gate + 1]
            if (fk == DEPOL1 and kind in ROT1 and fq0 == q0) or (fk == DEPOL2 and kind == CNOT and (fq0, fq1) == (q0, q1)):
                skip_end = new_gate + 2
    pre = []
    for i, (kind, q0, q1, pidx) in enumerate(gates):
        if skip <= i < skip_end:
            continue
        if kind in ROT1 + ROT2 and hole >= 0 and pidx > hole:
            pidx -= 1
        pre.append((kind, q0, q1, pidx))
    x0 = [theta[j] for j in range(P) if j != hole]
    it = iter(xopt)
    xraw = [theta[j] if j == hole else next(it) for j in range(P)]
    return (skip, skip_end, hole), pre, x0, xraw


def _bits(v):
    """16 hex digits: the double's bit pattern, as the checker reads and prints it."""
    return f"{struct.unpack('<Q', struct.pack('<d', float(v)))[0]:016x}"


def test_pre_action_circuit_and_merge(checker, tmp_path):
    cases = _make_cases()
    rng = np.random.default_rng(7)
    path = tmp_path / "cases.txt"
    want = []
    kinds_seen, final_pair_seen = set(), set()      # (new kind, gates left out), all cases / follower is the final gate
    with open(path, "w") as f:
        for c, (gates, P, new_gate) in enumerate(cases):
            theta = rng.uniform(-np.pi, np.pi, P)
            xopt = rng.uniform(-np.pi, np.pi, P)
            f.write(f"{len(gates)} {P} {new_gate}\n")
            for g in gates:
                f.write("%d %d %d %d\n" % tuple(g))
            f.write(" ".join(_bits(v) for v in theta) + "\n" + " ".join(_bits(v) for v in xopt) + "\n")
            (skip, skip_end, hole), pre, x0, xraw = _expected(gates, P, new_gate, theta, xopt)
            if new_gate >= 0:
                kinds_seen.add((gates[new_gate][0], skip_end - skip))
                if new_gate == len(gates) - 2:
                    final_pair_seen.add((gates[new_gate][0], skip_end - skip))
            x32 = [float(np.float32(v)) for v in xraw]
            assert all(a != b for a, b in zip(x32, xraw)), "the float32 rounding must be visible in every entry"
            want += [f"case {c} {skip} {skip_end} {hole}",
                     " ".join(["gates"] + [str(v) for g in pre for v in g]),
                     " ".join(["x0"] + [_bits(v) for v in x0]),
                     " ".join(["xraw"] + [_bits(v) for v in xraw]),
                     " ".join(["x32"] + [_bits(v) for v in x32]),
                     " ".join(["x64"] + [_bits(v) for v in xraw])]
    want.append("ok")
    # the cases do reach both outcomes where the rule allows both, and only one where it does not
    assert {(k, 2) for k in (CNOT,) + ROT1} <= kinds_seen and not any((k, 2) in kinds_seen for k in ROT2 + (DEPOL1, DEPOL2))
    assert {(k, 1) for k in range(9)} <= kinds_seen
    assert final_pair_seen == {(k, 1) for k in range(9)} | {(k, 2) for k in (CNOT,) + ROT1}
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=60)
    got = r.stdout.splitlines()
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for line, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"output line {line} (case {line // 6}: {cases[line // 6]}): got {g!r}, want {w!r}"
    assert len(got) == len(want)
