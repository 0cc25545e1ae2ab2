"""CPU: what the streaming path's quantum-jump trajectories (csrc/vqe_stream_qjump.h, vqe_set_stream_kraus_traj) can be
held to without a GPU.

* the preconditions of the GPU tests (tests/test_stream_kraus_traj_gpu.py) on the oracle (tests/qj_oracle.py) alone, for
  their exact cases: every draw at least 1e-9 from a boundary of its cumulative distribution and - the parity cases -
  every Kraus index of both sets chosen, no trajectory left out;
* tests/cpp/sq_host_check.cpp, built with g++ -fsanitize=address,undefined and run as a program: the host sizing of the
  lock-step loop (rounds, sweeps per round) against a brute-force walk, and the record ranges of the rounds;
* the ABI: the two symbols of the built library, the convention of max_resident in the header's text."""
import ctypes
import os
import subprocess

import pytest

import dm_kraus_oracle as ko
import qj_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sq_host_check.cpp")
LIB = os.path.join(ROOT, "tensorrl-qas_amd", "libvqe_hip.so")


@pytest.mark.parametrize("name", qc.COMBOS)
@pytest.mark.parametrize("n", [14, 15])
def test_parity_preconditions_hold_on_the_oracle(n, name):
    psi0, ham, circuits = qc.parity_case(n)
    K1, K2 = qc.combo(name)
    runs = qc.oracle_runs(psi0, ham, circuits, K1, K2, qc.PARITY_SEED, qc.PARITY_EVALS, qc.PARITY_T)
    qc.assert_preconditions(runs, K1, K2)
    print(f"n={n} {name}: smallest margin {min(r['margin'] for ev in runs for r in ev):.2e}")
    assert set(int(v) for c in circuits for v in c[0]) == set(range(9))


def test_cross_path_case_has_no_marginal_draw():
    """qc.parity_case(13) under damping+product, evaluations 0 - 2: the case both device paths run"""
    psi0, ham, circuits = qc.parity_case(13)
    K1, K2 = qc.combo("damping+product")
    runs = qc.oracle_runs(psi0, ham, circuits, K1, K2, qc.PARITY_SEED, 3, qc.PARITY_T)
    qc.assert_preconditions(runs, K1, K2)


def test_slot_cases_have_no_marginal_draw():
    n = 14
    psi0, ham, circuits = qc.parity_case(n)
    K2 = qc.combo("dephasing+cnot")[1]
    for K1r, K2r in ((ko.depol1(0.2), K2), (qc.amplitude_damping(0.3), None), (qc.amplitude_damping(0.3), ko.depol2(0.3))):
        runs = qc.oracle_runs(psi0, ham, circuits, K1r, K2r, 77, 1, 4)[0]
        assert min(r["margin"] for r in runs) >= qc.MARGIN
        assert sum(r["jumps"] for r in runs) > 0


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_qjump") / "sq_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"), SRC, "-o", str(exe)],
                   check=True)
    return str(exe)


def test_host_sizing_and_round_ranges(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.strip()}
    assert int(out["batches"][0]) >= 500 and int(out["batches"][2]) >= 1


def test_abi_symbols_and_header():
    header = open(os.path.join(ROOT, "include", "vqe_hip.h")).read()
    for text in ("int vqe_set_stream_kraus_traj(vqe_t* h, int max_resident);", "int vqe_stream_kraus_traj_info(vqe_t* h, int64_t out[4]);",
                 "0 (default) off", "-1 on, with", "a quarter of the free device memory at the first run", "R >= 1 on, with at most R resident",
                 "< -1 VQE_EINVAL"):
        assert text in header, text
    lib = ctypes.CDLL(LIB)
    for name in ("vqe_set_stream_kraus_traj", "vqe_stream_kraus_traj_info"):
        assert hasattr(lib, name), name
    lib.vqe_set_stream_kraus_traj.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.vqe_stream_kraus_traj_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
    assert lib.vqe_set_stream_kraus_traj(None, -1) == -22      # (a NULL handle is VQE_EINVAL, as for every setter)
    assert lib.vqe_stream_kraus_traj_info(None, (ctypes.c_int64 * 4)()) == -22
