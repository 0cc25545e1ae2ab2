"""CPU: the oracle of the quantum-jump trajectories (tests/qj_oracle.py) and the host parts of csrc/vqe_qjump.h.

* the oracle against the exact channel: the n = 3 circuit of test_noise_statistics_match_depolarizing_channels under
  amplitude damping and a product channel, 6 evaluations x 4096 trajectories - the mean within 3 sem (the oracle's own
  sample) of tests/dm_kraus_oracle.py;
* the oracle against the C oracle's Pauli path: with depolarising Kraus sets its states are vo.run_circuit's with the
  Paulis its chosen k name, to 1e-13;
* the preconditions of the GPU parity test (tests/test_kraus_traj_gpu.py) on the oracle alone: every draw at least 1e-9
  from a boundary, every Kraus index chosen, no trajectory left out;
* tests/cpp/qj_host_check.cpp, built with g++ -fsanitize=address,undefined and run as a program: the M_k tables and the
  compile walk (its header lists the bounds);
* the ABI: the three symbols, and the bounds of vqe_set_kraus_traj in the header's text."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dm_kraus_oracle as ko
import qj_cases as qc
import qj_oracle as qo
import vqe_oracle as vo
from dm_batch_cases import noisy
from helpers import random_gates, random_hamiltonian, random_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "qj_host_check.cpp")
LIB = os.path.join(ROOT, "tensorrl-qas_amd", "libvqe_hip.so")


def test_hash_restatement_matches_the_c_oracle():
    import c_oracle as co
    lib = co.lib()
    lib.orc_noise_uniform.restype = ctypes.c_double
    lib.orc_noise_uniform.argtypes = [ctypes.c_uint64] * 4
    for seed, b, e, g in ((0, 0, 0, 0), (424242, 3, 17, 5), (2 ** 64 - 1, 4095, 2 ** 40, (9 << 44) | 12345)):
        assert qo.noise_uniform_k(qo.noise_key(seed, b, e), g) == lib.orc_noise_uniform(seed, b, e, g)
    assert qo.draw(7, 1, 2, 0, 5) == qo.noise_uniform_k(qo.noise_key(7, 1, 2), (1 << 44) | 5)


def test_oracle_mean_is_the_exact_channel():
    psi0, ham, c = qc.dist_case()
    K1, K2 = qc.combo("damping+product")
    exact = ko.circuit_energy(psi0, c[0], c[1], c[2], c[3], c[4], K1, K2, ham)
    runs = qc.oracle_runs(psi0, ham, [c], K1, K2, qc.DIST_SEED, qc.DIST_EVALS, qc.DIST_T)
    s = np.concatenate([r[0]["energies"] for r in runs])
    sem = s.std() / np.sqrt(s.size)
    print(f"mean {s.mean():.6f} exact {exact:.6f} sem {sem:.2e} ({(s.mean() - exact) / sem:+.2f} sem)")
    assert s.size == 6 * 4096 and sem > 0
    assert abs(s.mean() - exact) < 3 * sem, (s.mean(), exact, sem)
    for r in runs:      # normalised states, the mean in t order
        assert np.abs(np.linalg.norm(r[0]["states"], axis=1) - 1).max() < 1e-13
        assert abs(r[0]["mean"] - r[0]["energies"].mean()) < 1e-13


@pytest.mark.parametrize("n", [2, 3, 4])
def test_depolarising_sets_follow_the_pauli_path(n):
    """k names the Pauli: I, X, Y, Z in the one-qubit slot, P_b (x) P_a at k = a + 4 b in the two-qubit slot - the codes
    vo.run_circuit takes as noise draws."""
    rng = np.random.default_rng(6100 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 10, rng, real=False)
    k, a, b, p, th = noisy(random_gates(n, 14, rng))
    T = 16
    r = qo.run(psi0, k, a, b, p, th, ko.depol1(0.3), ko.depol2(0.5), ham, 99, 2, 5, T)
    slots = np.nonzero((k == 4) | (k == 5))[0]
    assert r["ks"].shape == (T, slots.size) and r["jumps"] > T
    for t in range(T):
        draws = np.zeros(k.size, np.int64)
        draws[slots] = r["ks"][t]
        want = vo.run_circuit(psi0, k, a, b, p, th, draws)
        assert np.abs(r["states"][t] - want).max() <= 1e-13
        assert abs(r["energies"][t] - vo.energy_pauli(want, *ham)) <= 1e-13 * max(1.0, np.abs(ham[2]).sum())


@pytest.mark.parametrize("name", qc.COMBOS)
@pytest.mark.parametrize("n", [2, 5, 7, 9])
def test_parity_preconditions_hold_on_the_oracle(n, name):
    """(the sizes that take well under a second here; tests/test_kraus_traj_gpu.py asserts the same at every size)"""
    psi0, ham, circuits = qc.parity_case(n)
    K1, K2 = qc.combo(name)
    runs = qc.oracle_runs(psi0, ham, circuits, K1, K2, qc.PARITY_SEED, qc.PARITY_EVALS, qc.PARITY_T)
    qc.assert_preconditions(runs, K1, K2)
    kinds = set(int(v) for c in circuits for v in c[0])
    assert kinds == set(range(9)) or n < 2


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("qjump") / "qj_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"), SRC, "-o", str(exe)],
                   check=True)
    return str(exe)


def test_tables_and_compile_walk(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.strip()}
    assert float(out["tables"][0]) <= 1e-14 and float(out["depol"][0]) == 0.0
    assert float(out["walk"][0]) <= 1e-13 and float(out["walk"][2]) <= 1e-13 and int(out["walk"][4]) == 36


def test_abi_symbols():
    """the three entry points are exported; the bounds of vqe_set_kraus_traj are enforced before the handle is touched
    (a NULL handle is VQE_EINVAL, as for every setter; with a device: tests/test_kraus_traj_gpu.py)"""
    lib = ctypes.CDLL(LIB)
    for name in ("vqe_set_kraus_traj", "vqe_kraus_traj_info", "vqe_batch_fetch_traj"):
        assert hasattr(lib, name), name
    lib.vqe_set_kraus_traj.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.vqe_set_kraus_traj(None, 4) == -22
    header = open(os.path.join(ROOT, "include", "vqe_hip.h")).read()
    for name in ("int vqe_set_kraus_traj(vqe_t* h, int n_traj);", "int vqe_kraus_traj_info(vqe_t* h, int64_t out[4]);",
                 "int vqe_batch_fetch_traj(vqe_t* h, double* e"):
        assert name in header, name
