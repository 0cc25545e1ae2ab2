"""CPU: gradients of frozen Pauli-noise realisations (vqe_set_noise_grad) - everything that needs no device.
* the ABI: the three functions in the header (the definition's words among them) and in the library, a NULL handle
  refused; the Python wrappers exist;
* tests/cpp/noise_grad_check.cpp, built with g++ -fsanitize=address,undefined and run as a program: the verdict and the
  counter rules of csrc/noise_grad_host.h driven through call sequences and compared with the rules as include/vqe_hip.h
  states them, restated below (`Model`); a refused call changes nothing;
* the reference itself: the parameter shift of tests/noise_grad_cases.py on a noiseless realisation equals the project's
  noiseless shift gradient;
* the preconditions of tests/test_noise_grad_gpu.py on the CPU oracle alone: what the draws of the parity cases contain,
  and the 4 sigma statement of the statistics case."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import noise_grad_cases as ngc
import noise_pauli_oracle as npo
from helpers import shift_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "noise_grad_check.cpp")
LIB = os.path.join(ROOT, "tensorrl-qas_amd", "libvqe_hip.so")


def test_abi():
    header = open(os.path.join(ROOT, "include", "vqe_hip.h")).read()
    for text in ("int vqe_set_noise_grad(vqe_t* h, int n_real, int hold);", "int vqe_noise_grad_advance(vqe_t* h);",
                 "int vqe_noise_grad_info(vqe_t* h, int64_t out[4]);", "summed in ascending t",
                 "The result has the same bits for the same (seed, eval_base, batch position, T)."):
        assert text in header, text
    lib = ctypes.CDLL(LIB)
    for name in ("vqe_set_noise_grad", "vqe_noise_grad_advance", "vqe_noise_grad_info"):
        assert hasattr(lib, name), name
    lib.vqe_set_noise_grad.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.vqe_noise_grad_advance.argtypes = [ctypes.c_void_p]
    lib.vqe_noise_grad_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    out = (ctypes.c_int64 * 4)()
    assert lib.vqe_set_noise_grad(None, 4, 0) == -22 and lib.vqe_noise_grad_advance(None) == -22
    assert lib.vqe_noise_grad_info(None, out) == -22
    import tensorrl_qas_amd as tq
    for name in ("set_noise_grad", "noise_grad_advance", "noise_grad_info"):
        assert callable(getattr(tq.VQEEngine, name)), name


# ---- the rules as the header states them ---------------------------------------------------------------------------------
class Model:
    def __init__(self):
        self.T, self.hold, self.pauli, self.mode, self.n, self.shot, self.shard, self.base = 0, False, False, 0, 8, 0, 1, 0

    def run(self, op, a, b):
        """-> return code of the model (0 served / done, else refused)"""
        if op == "new":
            self.__init__()
        elif op == "set":
            if not 0 <= a <= 4096:
                return -22
            self.T, self.hold = a, bool(b)
        elif op == "noise":
            self.pauli, self.base = bool(a), 0
        elif op == "mode":
            self.mode = a
        elif op == "qubits":
            self.n = a
        elif op == "shot":
            self.shot = a
        elif op == "shard":
            self.shard = a
        elif op == "advance":
            self.base += self.T
        else:
            on = self.pauli and self.T > 0 and self.mode == 0
            if self.pauli and not on:
                return 1
            if on and self.n >= 14:
                return 2
            if self.mode == 1:
                return 3
            if self.shot:
                return 4
            if op != "grad" and self.shard > 1:
                return 5
            if on:
                self.base += {"grad": 0 if self.hold else self.T, "lbfgs": self.T, "envstep": self.T + 1}[op]
        return 0


SCRIPTS = {
    "off_by_default": [("noise", 1, 0), ("grad", 0, 0), ("lbfgs", 0, 0), ("envstep", 0, 0)],
    "noiseless_whatever_the_switch": [("set", 8, 0), ("grad", 0, 0), ("lbfgs", 0, 0), ("envstep", 0, 0), ("advance", 0, 0)],
    "counter": [("noise", 1, 0), ("set", 5, 0), ("grad", 0, 0), ("grad", 0, 0), ("lbfgs", 0, 0), ("envstep", 0, 0),
                ("set", 5, 1), ("grad", 0, 0), ("grad", 0, 0), ("advance", 0, 0), ("grad", 0, 0), ("lbfgs", 0, 0),
                ("envstep", 0, 0), ("set", 0, 0), ("grad", 0, 0), ("advance", 0, 0)],
    "bad_counts_change_nothing": [("noise", 1, 0), ("set", 7, 1), ("set", -1, 0), ("set", 4097, 0), ("grad", 0, 0),
                                  ("advance", 0, 0), ("set", 4096, 0), ("grad", 0, 0)],
    "refusals_change_nothing": [("noise", 1, 0), ("set", 3, 0), ("grad", 0, 0), ("mode", 1, 0), ("grad", 0, 0), ("lbfgs", 0, 0),
                                ("mode", 0, 0), ("shot", 1, 0), ("grad", 0, 0), ("envstep", 0, 0), ("shot", 0, 0),
                                ("shard", 2, 0), ("grad", 0, 0), ("lbfgs", 0, 0), ("envstep", 0, 0), ("shard", 1, 0),
                                ("qubits", 14, 0), ("grad", 0, 0), ("lbfgs", 0, 0), ("qubits", 13, 0), ("lbfgs", 0, 0)],
    "set_noise_resets_the_counter": [("noise", 1, 0), ("set", 2, 0), ("grad", 0, 0), ("noise", 1, 0), ("grad", 0, 0)],
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("noise_grad") / "noise_grad_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"), SRC, "-o", str(exe)],
                   check=True)
    return str(exe)


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_verdict_and_counter_rules(checker, tmp_path, name):
    script = [("new", 0, 0)] + SCRIPTS[name]
    path = tmp_path / "script.txt"
    path.write_text("".join(f"{op} {a} {b}\n" for op, a, b in script))
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")[:len(script)]
    m, served, refused = Model(), 0, 0
    for (op, a, b), ln in zip(script, lines):
        before = (m.T, m.hold, m.base)
        rc = m.run(op, a, b)
        assert ln.split() == [op, str(rc), str(m.base)], (name, op, a, b, ln)
        if rc != 0:
            assert (m.T, m.hold, m.base) == before      # a refused call changes nothing
            refused += 1
        elif op in ("grad", "lbfgs", "envstep"):
            served += 1
    if name in ("off_by_default",):
        assert served == 0 and refused == 3
    if name == "counter":
        assert refused == 1 and m.base == 5 + 5 + 5 + 6 + 5 + 5 + 6        # (the last grad: switch off again, refused)
    if name == "refusals_change_nothing":
        assert served == 3 and refused == 8 and m.base == 3 + 3 + 3


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_reference_without_errors_is_the_noiseless_shift_gradient():
    case = ngc.parity_case(3)
    (kind, q0, q1, pidx), th = case["circuits"][0]
    keep = kind < 4
    e, g = ngc.realisation(case["psi0"], (kind, q0, q1, pidx), th, case["ham"], np.zeros(kind.size, np.int64))
    ref = shift_grad(case["psi0"], kind[keep], q0[keep], q1[keep], pidx[keep], th, case["ham"])
    assert np.abs(g - ref).max() <= 1e-12 * case["scale"]
    # ... and a Z error in front of a rotation about X changes it (the codes reach the reference)
    g_first = int(np.flatnonzero(kind == npo.DEPOL1)[0])
    codes = np.zeros(kind.size, np.int64)
    codes[g_first] = 3
    assert np.abs(ngc.realisation(case["psi0"], (kind, q0, q1, pidx), th, case["ham"], codes)[1] - ref).max() > 1e-3


def test_preconditions_of_the_parity_cases():
    """the draws of the checked realisations contain together: one without an error, an X or Y error on the control in
    front of a CNOT, a Y, an error on both qubits of a two-qubit slot; no draw sits on a threshold; the patch crosses
    its 64-gate chunk; RXX / RYY / RZZ are present at n = 9."""
    assert ngc.parity_features() == {"none", "x_before_control", "y", "both"}
    for n in ngc.PARITY_N:
        case = ngc.parity_case(n)
        assert ngc.parity_codes(case)[1] > 1e-12
        assert max(c[0][0].size for c in case["circuits"]) == 2 * ngc.G_LONG > 64
    assert {6, 7, 8} <= set(int(k) for c in ngc.parity_case(9)["circuits"] for k in c[0][0])


def test_preconditions_of_the_statistics_case():
    """n = 3, 64 positions x T = 64: the CPU oracle's block means lie within 4 sigma of the exact channel gradient, and
    that gradient is far from the noiseless one in units of sigma somewhere (the statement is about the noise)."""
    c = ngc.stat_case()
    exact = ngc.stat_exact_grad(c)
    ok, m, s = ngc.within_4_sigma(ngc.stat_oracle_blocks(c), exact)
    print("exact", exact, "mean", m, "sigma", s)
    assert ok
    clean = ngc.realisation(c["psi0"], c["gates"], c["theta"], c["ham"], np.zeros(c["gates"][0].size, np.int64))[1]
    assert np.max(np.abs(clean - exact) / s) >= 10
