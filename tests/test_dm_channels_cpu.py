"""CPU: Kraus channels in the noise slots of the exact channel mode and two-qubit rotations as block members (DESIGN
4.16) - the host maths and the Python side, without a GPU.

* tests/dm_kraus_oracle.py (explicit Kraus sums on a dense rho) with depolarising Kraus sets against the oracle's own
  channel vo.run_circuit_dm, <= 1e-13: ties the helper the GPU tests rely on to the one the project already trusts.
* tensorrl_qas_amd.channels: every generator is trace preserving, amplitude damping and the product channel do what
  their names say, independent_xz is a bit flip composed with a dephasing.
* tests/cpp/dm_channel_check.cpp (a plain host program, built here with g++): the Kraus tables against sup_depol, the
  orientation of the two-qubit table, the two-qubit rotation members against the fill, the derivative chain through
  them against the exact shift, and today's plans unchanged without an override (its header lists the bounds)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import dm_kraus_oracle as ko
import vqe_oracle as vo
from dm_batch_cases import noisy
from helpers import random_gates, random_hamiltonian, random_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dm_channel_check.cpp")


@pytest.fixture(scope="module")
def ch():
    """channels.py on its own: host only, importable without the compiled library"""
    spec = importlib.util.spec_from_file_location("_channels_under_test", os.path.join(ROOT, "tensorrl-qas_amd", "channels.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n", [2, 3, 4])
def test_helper_with_depolarising_sets_equals_the_oracle_channel(n):
    rng = np.random.default_rng(5200 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 12, rng, real=False)
    for G, p1, p2 in ((1, 0.3, 0.2), (9, 0.01, 0.05), (16, 0.2, 0.6)):
        k, a, b, p, th = noisy(random_gates(n, G, rng))
        want = vo.run_circuit_dm(psi0, k, a, b, p, th, p1, p2)
        got = ko.run(psi0, k, a, b, p, th, ko.depol1(p1), ko.depol2(p2))
        assert np.abs(got - want).max() <= 1e-13
        assert abs(ko.energy(got, *ham) - vo.energy_dm(want, *ham)) <= 1e-13 * max(1.0, np.abs(ham[2]).sum())
    assert np.any(k == 5) and np.any(k == 4)


def test_helper_two_qubit_rotations_and_shift_rule():
    """exp(i theta/2 P P) against the state-vector definition, and the shift gradient against central differences"""
    n = 3
    rng = np.random.default_rng(5210)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 10, rng, real=False)
    for kind in (ko.RXX, ko.RYY, ko.RZZ):
        u = ko.rot2(n, kind, 2, 0, 0.7)
        pp = ko.embed1(n, 2, ko.PAULI[kind - 5]) @ ko.embed1(n, 0, ko.PAULI[kind - 5])
        w, v = np.linalg.eigh(pp)
        assert np.abs(u - (v * np.exp(0.35j * w)) @ v.conj().T).max() <= 1e-14
        assert np.abs(u - ko.rot2(n, kind, 0, 2, 0.7)).max() == 0.0
    circ = (np.array([1, 4, 6, 5, 0, 5, 8, 2, 4], np.int32), np.array([0, 0, 0, 0, 1, 1, 2, 2, 2], np.int32),
            np.array([-1, -1, 2, 2, 2, 2, 1, -1, -1], np.int32), np.array([0, -1, 1, -1, -1, -1, 2, 3, -1], np.int32))
    th = rng.uniform(-np.pi, np.pi, 4)
    K1, K2 = np.array([[[1, 0], [0, np.sqrt(0.7)]], [[0, np.sqrt(0.3)], [0, 0]]]), ko.depol2(0.1)
    g = ko.shift_grad(psi0, *circ, th, K1, K2, ham)
    h = 1e-5
    for j in range(4):
        d = np.zeros(4)
        d[j] = h
        fd = (ko.circuit_energy(psi0, *circ, th + d, K1, K2, ham) - ko.circuit_energy(psi0, *circ, th - d, K1, K2, ham)) / (2 * h)
        assert abs(fd - g[j]) <= 1e-8 * max(1.0, np.abs(ham[2]).sum())
    assert np.abs(g).max() > 1e-3


def _apply(K, rho):
    return sum(m @ rho @ m.conj().T for m in K)


def test_channel_generators(ch):
    for p in (0.0, 0.01, 0.3, 1.0):
        sets = [ch.depolarizing(p), ch.two_qubit_depolarizing(p), ch.amplitude_damping(p), ch.dephasing(p), ch.bit_flip(p),
                ch.independent_xz(p), ch.tensor(ch.amplitude_damping(p), ch.dephasing(0.2)), ch.identity(2), ch.identity(4)]
        for K in sets:
            assert K.dtype == np.complex128 and K.ndim == 3 and K.shape[1] == K.shape[2] and ch.is_trace_preserving(K)
        assert sets[0].shape == (4, 2, 2) and sets[1].shape == (16, 4, 4) and sets[6].shape == (4, 4, 4)
        assert np.abs(sets[0] - ko.depol1(p)).max() <= 1e-16 and np.abs(sets[1] - ko.depol2(p)).max() <= 1e-16
    assert not ch.is_trace_preserving(0.9 * ch.dephasing(0.1))
    assert not ch.is_trace_preserving(ch.amplitude_damping(0.3)[:1])
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            ch.amplitude_damping(bad)
    one = np.diag([0.0, 1.0]).astype(np.complex128)
    for g in (0.0, 0.25, 1.0):
        assert np.abs(_apply(ch.amplitude_damping(g), one) - np.diag([g, 1.0 - g])).max() <= 1e-15
    rng = np.random.default_rng(5220)
    v = random_state(1, rng)
    rho = np.outer(v, v.conj())
    X, Z = np.array([[0, 1], [1, 0]]), np.diag([1.0, -1.0])
    for p in (0.1, 0.5):
        assert np.abs(_apply(ch.dephasing(p), rho) - ((1 - p) * rho + p * Z @ rho @ Z)).max() <= 1e-15
        assert np.abs(_apply(ch.bit_flip(p), rho) - ((1 - p) * rho + p * X @ rho @ X)).max() <= 1e-15
        both = _apply(ch.dephasing(p), _apply(ch.bit_flip(p), rho))
        assert np.abs(_apply(ch.independent_xz(p), rho) - both).max() <= 1e-15
        assert np.abs(_apply(ch.bit_flip(p), _apply(ch.dephasing(p), rho)) - both).max() <= 1e-15
    # tensor(Ka, Kb): Ka on q0 = the low index bit
    w = random_state(2, rng)
    rho2 = np.outer(w, w.conj())
    K = ch.tensor(ch.amplitude_damping(1.0), ch.identity(2))
    out = _apply(K, rho2)
    assert abs(out[1, 1]) + abs(out[3, 3]) <= 1e-15                                   # q0 ends in |0>
    assert abs(out[0, 0] - (rho2[0, 0] + rho2[1, 1])) <= 1e-15 and abs(out[2, 2] - (rho2[2, 2] + rho2[3, 3])) <= 1e-15
    with pytest.raises(ValueError):
        ch.tensor(ch.identity(4), ch.identity(2))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dmchan") / "dm_channel_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def test_tables_members_derivatives_and_plans(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.strip()}
    print(r.stdout)
    assert float(out["kraus"][0]) <= 1e-15 and float(out["chain"][0]) <= 1e-14 and float(out["derivative"][0]) <= 1e-13
    first = r.stdout.splitlines()[0].split()      # "blocks B rot2 R swapped S derivatives D"
    counts = dict(zip(first[0::2], (int(v) for v in first[1::2])))
    assert counts["rot2"] > 20 and counts["swapped"] > 5 and counts["derivatives"] > 50
