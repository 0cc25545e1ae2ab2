"""CPU: the plan / fill split of the exact channel mode's block builder (csrc/dm_host.h) and the per-block builder the
batched kernels compile (csrc/dm_build.h).

tests/cpp/dm_plan_check.cpp (a plain host program, built here with g++) holds, for every circuit of a batch,
(i) dm_plan_blocks + dm_fill_blocks, and dm_make_blocks on top of them, against the one-pass builder from before the
split - same windows, same bits of every matrix; (ii) the shared builder dm_build_entry against the fill, <= 1e-14 per
entry (members in list order, inner index ascending, identity start - the order k_dm_build runs on the device);
(iii) the flattened device tables: every block and every member addressed exactly once by the per-circuit block ranges and
the per-block member ranges, the four window index bits ascending.

Circuits: random_gates with a channel behind every gate at n = 2, 3, 5, 8, 12 with 0, 1 and many gates, plus circuits
whose one-qubit gates open their window with each of the three partner rules (the partner named by the next two-qubit
gate, any free qubit, the oldest block evicted); the program counts the rules it met."""
import os
import subprocess

import numpy as np
import pytest

from dm_batch_cases import gate_list, mixed_batch, noisy
from helpers import random_gates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dm_plan_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dmplan") / "dm_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def _run(checker, tmp_path, n, circuits, p1=0.07, p2=0.11):
    """-> (blocks per circuit, rule counts (next two-qubit gate, free qubit, evicted), max |builder - fill|)"""
    path = str(tmp_path / "circuits.txt")
    with open(path, "w") as f:
        f.write(f"{n} {float(p1).hex()} {float(p2).hex()} {len(circuits)}\n")
        for kind, q0, q1, pidx, th in circuits:
            f.write(f"{len(kind)} {len(th)}\n")
            for g in zip(kind, q0, q1, pidx):
                f.write(" ".join(str(int(v)) for v in g) + "\n")
            f.write(" ".join(float(t).hex() for t in th) + "\n")
    r = subprocess.run([checker, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.strip()}
    blocks = [int(v) for v in out["blocks"]]
    assert len(blocks) == len(circuits)
    return blocks, tuple(int(v) for v in out["rules"]), float(out["maxdiff"][0])


@pytest.mark.parametrize("n", [2, 3, 5, 8, 12])
def test_plan_fill_and_builder_on_random_circuits(checker, tmp_path, n):
    rng = np.random.default_rng(4100 + n)
    circuits = [noisy(random_gates(n, G, rng)) for G in (0, 1, 1, 7, 40)] + mixed_batch(n, 24, rng)
    circuits.append(noisy(random_gates(n, 30, rng, p_cnot=0.15)))      # mostly one-qubit gates: windows opened by the partner rules
    blocks, rules, diff = _run(checker, tmp_path, n, circuits)
    assert blocks[0] == 0 and blocks[1] == 1 and blocks[2] == 1 and blocks[7] == 0
    assert all(1 <= b <= 80 for b in blocks[3:5])
    assert diff <= 1e-14
    assert rules[0] > 0 and rules[1] > 0
    if n in (3, 5):          # an odd qubit is left over when every other one sits in a window
        assert rules[2] > 0, rules


def test_every_partner_rule_by_construction(checker, tmp_path):
    """One circuit per rule on 3 qubits, each meeting its rule and no other."""
    next_2q = gate_list([(1, 0, -1, 0.3), (0, 2, 0, None)])                         # RX(0), then CNOT(2, 0): window (0, 2)
    free = gate_list([(0, 0, 1, None), (2, 2, -1, -0.4), (2, 2, -1, 1.4)])         # (0, 1) open, RY(2): no later two-qubit gate ...
    evict = gate_list([(0, 0, 1, None), (3, 2, -1, 0.9)])                          # ... and no free qubit: the oldest block goes
    for circ, want, nblocks in ((next_2q, (1, 0, 0), 1), (evict, (0, 0, 1), 2)):
        blocks, rules, _ = _run(checker, tmp_path, 3, [noisy(circ)])
        assert rules == want and blocks == [nblocks], (rules, blocks)
    blocks, rules, _ = _run(checker, tmp_path, 4, [noisy(free)])                   # on 4 qubits qubit 3 is free
    assert rules == (0, 1, 0) and blocks == [2]


def test_high_window_bits_and_strong_channels(checker, tmp_path):
    """n = 12 windows (10, 11) and (0, 11) beside an open block; p = 1 and p = 0 channels."""
    circ = gate_list([(0, 4, 5, None), (1, 10, -1, 0.7), (0, 10, 11, None), (3, 11, -1, -1.1), (0, 11, 0, None), (2, 0, -1, 0.2),
                      (1, 5, -1, 2.0), (0, 0, 11, None)])
    for p1, p2 in ((0.0, 0.0), (1.0, 1.0), (0.01, 0.05)):
        blocks, _, diff = _run(checker, tmp_path, 12, [noisy(circ), circ], p1, p2)
        assert blocks[0] == blocks[1] and diff <= 1e-14
