"""CPU: the planner of the MPS -> PQC fit (csrc/mps2qc_plan.h) against the contract k_fit relies on.

tests/cpp/mps2qc_plan_check.cpp plans, with the library's own planner (a host-only header, built here with g++),
brickwork circuits of 2..12 qubits and 1..8 layers and gate sequences with repeated and overlapping pairs, each with
the half-layer scheme on / off and with / without the two-buffer knob, and checks EXACTLY - no tolerance:

1. runs: an ordered partition of the gates, pairwise disjoint within a run, every run maximal;
2. LDS layout: every region the kernel touches (psi/phi, U, E, red x red_slots, sc, dn, lo, grp, scratch) inside the
   total, aligned for its element type and disjoint from every other - but for the scratch overlay on psi/phi, which
   is there (off_scratch == 0) exactly when the two states are at least as large as the scratch;
3. the total is <= 160 KiB, otherwise the planner refuses with a message;
4. red_slots: the largest run (never fewer than the two the kernel double-buffers with) when the half-layer scheme
   runs, the two-buffer knob is off and it fits; otherwise 2;
5. three layouts at 12 qubits to the byte (1 layer: six buffers; 4 layers: back to two; 6 layers: refused);
6. argument checks and their messages, lo[k] = n - 2 - sites[k], threads per fit;
7. the learning-rate schedule: frozen = step 1 at every step, otherwise lr sqrt(1 - b2^t) / (1 - b1^t) bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mps2qc_plan_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "mps2qc_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True, timeout=300)
    return str(exe)


def test_planner_contract(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    planned, refused = (int(w) for w in r.stdout.splitlines()[-2].split()[1::2])
    # 88 brickwork circuits + 18 sequences, four knob settings each; some 12-qubit circuits must be refused
    assert planned + refused == 4 * (11 * 8 + 18) and refused > 0 and planned > 300
