"""CPU: the RXX / RYY / RZZ gate kinds through the host layers - ABI constants, the QASM reader, the SU(4) ansatz
builder, the amplitude-shard planner's refusal - and the reference the GPU tests (test_su4_gpu.py) compare with."""
import importlib
import os
import re

import numpy as np
import pytest

import vqe_oracle as vo
import su4_helpers as s4
from helpers import random_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gate_kind_constants_agree_with_the_header():
    import tensorrl_qas_amd as tq
    text = open(os.path.join(ROOT, "include", "vqe_hip.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"VQE_GATE_(\w+)\s*=\s*(\d+)", text)}
    assert vals == {"CNOT": 0, "RX": 1, "RY": 2, "RZ": 3, "DEPOL1": 4, "DEPOL2": 5, "RXX": 6, "RYY": 7, "RZZ": 8}
    for name, v in vals.items():
        assert getattr(tq.engine, "GATE_" + name) == v
    assert "VQE_qulacs_su4.py:68-90" in text


QASM = """OPENQASM 2.0;
include "qelib1.inc";
qreg q[4];
rxx(pi/2) q[0],q[1];
ry(0.25) q[2];
ryy(-0.75) q[3],q[1];
cx q[1],q[2];
rzz(3*pi/4 - 0.5) q[2], q[0];
rz(-pi) q[3];
"""


def test_qasm_reads_the_su4_basis():
    import tensorrl_qas_amd as tq
    n, gates = tq.qasm.parse(QASM)
    assert n == 4
    assert [(g.name, g.qubits) for g in gates] == [("rxx", (0, 1)), ("ry", (2,)), ("ryy", (3, 1)), ("cx", (1, 2)),
                                                    ("rzz", (2, 0)), ("rz", (3,))]
    circ, ang = tq.circuits.circuit_from_qasm_gates(gates)
    assert circ.kind.tolist() == [6, 2, 7, 0, 8, 3]
    assert circ.q0.tolist() == [0, 2, 3, 1, 2, 3]
    assert circ.q1.tolist() == [1, -1, 1, 2, 0, -1]
    assert circ.pidx.tolist() == [0, 1, 2, -1, 3, 4] and circ.n_params == 5
    assert np.allclose(ang, [-np.pi / 2, -0.25, 0.75, -(3 * np.pi / 4 - 0.5), np.pi], rtol=0, atol=1e-15)
    assert len(tq.qasm.layers(n, gates)) == 4
    head = "OPENQASM 2.0;\nqreg q[3];\n"
    for bad in ("rxx(0.1) q[0];", "ryy q[0],q[1];", "rzz(0.1) q[0],q[1],q[2];", "rxx(0.2) q[1],q[1];", "rx(0.1) q[0],q[1];"):
        with pytest.raises(ValueError):
            tq.qasm.parse(head + bad)


def test_qasm_counts_of_the_shipped_su4_circuit_when_the_reference_is_present():
    import glob
    import tensorrl_qas_amd as tq
    ref = os.environ.get("TENSORRL_QAS_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
    files = glob.glob(os.path.join(ref, "dmrg-to-qc", "init_state_circ", "init_CH2_10q_*_TNbond5_su4.qasm"))
    if not files:
        pytest.skip("reference checkout not present")
    n, gates = tq.qasm.parse(open(files[0]).read())
    names = [g.name for g in gates]
    assert n == 10 and (names.count("rxx"), names.count("rz"), names.count("ry")) == (54, 236, 118)


def _su4_state(n, layers):
    """layers: per layer a list of (block, target_or_axis, control_or_qubit, angle), block 0..2 = xx / yy / zz, 3 = one-qubit."""
    s = np.zeros((len(layers), 6 * n + 6, n), np.float32)
    for li, items in enumerate(layers):
        for blk, t, c, ang in items:
            pos = blk * n + t if blk < 3 else 3 * n + t
            val = 3 * n + 3 + blk * n + t if blk < 3 else 6 * n + 3 + t
            s[li, pos, c] = 1
            s[li, val, c] = ang
    return s


def test_su4_construct_ansatz_order_and_angles():
    import torch
    su4 = importlib.import_module("tensorrl_qas_amd.environments.VQAs.VQE_qulacs_su4")
    n = 4
    layers = [
        # xx at [target 2][control 0] and [target 0][control 3]: row-major [target][control] puts (t=0, c=3) FIRST,
        # [control][target] order would put (c=0, t=2) first
        [(0, 2, 0, 0.11), (0, 0, 3, 0.12), (1, 1, 2, 0.21), (1, 1, 0, 0.22), (2, 3, 1, 0.31),
         (3, 2, 1, 0.41), (3, 0, 3, 0.42), (3, 0, 0, 0.43)],
        [(2, 0, 1, 0.51), (2, 0, 2, 0.52), (0, 3, 2, 0.61), (3, 1, 2, 0.71)],
    ]
    state = torch.from_numpy(_su4_state(n, layers))
    pc = su4.Parametric_Circuit(n)
    circ = pc.construct_ansatz(state)
    want = [  # (kind, q0 = control / qubit, q1 = target, angle)
        (6, 3, 0, 0.12), (6, 0, 2, 0.11), (7, 0, 1, 0.22), (7, 2, 1, 0.21), (8, 1, 3, 0.31),
        (1, 0, -1, 0.43), (1, 3, -1, 0.42), (3, 1, -1, 0.41),
        (6, 2, 3, 0.61), (8, 1, 0, 0.51), (8, 2, 0, 0.52), (2, 2, -1, 0.71)]
    assert list(zip(circ.kind.tolist(), circ.q0.tolist(), circ.q1.tolist())) == [w[:3] for w in want]
    assert circ.pidx.tolist() == list(range(len(want))) and circ.n_params == len(want)
    assert np.array_equal(circ.angles, np.array([w[3] for w in want], np.float32).astype(np.float64))
    assert np.array_equal(pc.angles, circ.angles)
    with pytest.raises(ValueError):
        pc.construct_ansatz(np.zeros((1, n + 6, n), np.float32))      # the CNOT gate set's tensor


def test_amplitude_shard_planner_refuses_the_new_kinds():
    from tensorrl_qas_amd import parallel
    for k in (6, 7, 8):
        with pytest.raises(NotImplementedError):
            parallel.plan_amplitude_sharding(4, 2, [1, k], [0, 1], [-1, 3], [0b11])
    parallel.plan_amplitude_sharding(4, 2, [1, 0], [0, 1], [-1, 3], [0b11])


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_expansion_agrees_with_the_definition(n):
    """R_PP(a, b, t) psi = cos(t/2) psi + i sin(t/2) P_a P_b psi, with P_a P_b psi from vqe_oracle.apply_pauli."""
    rng = np.random.default_rng(60 + n)
    for k in (6, 7, 8):
        for _ in range(6):
            a = int(rng.integers(n))
            b = int((a + 1 + rng.integers(n - 1)) % n)
            t = float(rng.uniform(-2 * np.pi, 2 * np.pi))
            psi = random_state(n, rng)
            got = s4.run_circuit(psi, [k], [a], [b], [0], np.array([t]))
            pp = vo.apply_pauli(vo.apply_pauli(psi, a, k - 5), b, k - 5)
            want = np.cos(t / 2) * psi + 1j * np.sin(t / 2) * pp
            assert np.abs(got - want).max() <= 1e-14, (n, k, a, b)
            # symmetric in (a, b)
            assert np.abs(s4.run_circuit(psi, [k], [b], [a], [0], np.array([t])) - want).max() <= 1e-14


def test_random_circuit_is_unchanged():
    import tensorrl_qas_amd as tq
    c, th = tq.circuits.random_circuit(5, 12, np.random.default_rng(3))
    # what the generator produced for this seed before the SU(4) kinds existed (the bench workload is drawn from it)
    assert c.kind.tolist() == [0, 3, 0, 0, 0, 2, 3, 2, 0, 0, 2, 2]
    assert c.q0.tolist() == [0, 2, 3, 3, 2, 2, 4, 3, 0, 0, 2, 0]
    assert c.q1.tolist() == [1, -1, 0, 1, 4, -1, -1, -1, 4, 2, -1, -1]
    assert th.size == 6 and abs(float(th.sum()) - -3.5429381065289762) < 1e-15


def test_qasm_still_reads_what_it_read_before():
    import tensorrl_qas_amd as tq
    n, gates = tq.qasm.parse("OPENQASM 2.0;\nqreg q[2];\ncx q[1],q[1];\nrz(pi) q[0];\n")      # (refused later, by the library)
    assert n == 2 and [(g.name, g.qubits) for g in gates] == [("cx", (1, 1)), ("rz", (0,))]
