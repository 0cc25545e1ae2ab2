"""CPU: gradients of frozen Pauli-noise realisations on the streaming path (vqe_set_stream_noise_grad) -
everything that needs no device.
* the ABI: the two functions in the header and in the library, a NULL handle refused; the Python wrappers exist;
* tests/cpp/stream_noise_grad_check.cpp, built with g++ -fsanitize=address,undefined and run as a program: the extended
  verdict of csrc/noise_grad_host.h (every old verdict with the streaming form off, the new one, mode 1 / switch off
  still refused as before) and the chunk planner of the (circuit, realisation) grid, compared with the rules restated
  below;
* the preconditions of tests/test_stream_noise_grad_gpu.py from the draws alone."""
import ctypes
import os
import subprocess

import pytest

import stream_noise_grad_cases as sng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stream_noise_grad_check.cpp")
LIB = os.path.join(ROOT, "tensorrl-qas_amd", "libvqe_hip.so")
NOISELESS, SERVED, REFUSED_OFF, REFUSED_PATH, SERVED_STREAM = 0, 1, 2, 3, 4


def test_abi():
    header = open(os.path.join(ROOT, "include", "vqe_hip.h")).read()
    for text in ("int vqe_set_stream_noise_grad(vqe_t* h, int max_resident);",
                 "int vqe_stream_noise_grad_info(vqe_t* h, int64_t out[4]);"):
        assert text in header, text
    lib = ctypes.CDLL(LIB)
    for name in ("vqe_set_stream_noise_grad", "vqe_stream_noise_grad_info"):
        assert hasattr(lib, name), name
    lib.vqe_set_stream_noise_grad.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.vqe_stream_noise_grad_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    out = (ctypes.c_int64 * 4)()
    assert lib.vqe_set_stream_noise_grad(None, 1) == -22 and lib.vqe_stream_noise_grad_info(None, out) == -22
    import tensorrl_qas_amd as tq
    for name in ("set_stream_noise_grad", "stream_noise_grad_info", "noise_grad_info"):
        assert callable(getattr(tq.VQEEngine, name)), name


# ---- the rules, restated --------------------------------------------------------------------------------------------------
def verdict(n_real, mode, pauli, lds, stream):
    if not pauli:
        return NOISELESS
    if n_real <= 0 or mode != 0:
        return REFUSED_OFF
    if lds:
        return SERVED
    return SERVED_STREAM if stream > 0 else REFUSED_PATH


def plan(B, T, cap):
    pairs = B * T
    resident = max(1, min(max(cap, 1), pairs, 65535))
    chunks = -(-pairs // resident)
    lines = [f"plan {pairs} {resident} {chunks}"]
    for c in range(chunks):
        lo, hi = c * resident, min((c + 1) * resident, pairs)
        lines.append(f"chunk {c} {lo} {hi} {lo // T} {lo % T} {(hi - 1) // T} {(hi - 1) % T}")
    return lines


VERDICTS = [(T, mode, pauli, lds, stream) for T in (0, 3) for mode in (0, 1) for pauli in (0, 1) for lds in (0, 1)
            for stream in (-1, 0, 1)]
PLANS = [(3, 3, 2),          # B T = 9 is no multiple of the resident count: a last chunk of one pair
         (3, 3, 4),          # a chunk boundary inside a circuit's realisations
         (2, 4, 8), (2, 4, 100),      # resident >= B T: one chunk
         (5, 3, 1),          # the serial form
         (1, 16, 16), (1, 1, 1), (7, 1, 3), (2, 3, 0), (2, 3, -1),      # (a cap below 1 plans as 1)
         (40, 4096, 1 << 20)]      # the y extent of a grid bounds a chunk


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_noise_grad") / "stream_noise_grad_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"), SRC, "-o", str(exe)],
                   check=True)
    return str(exe)


def _run(checker, tmp_path, lines):
    path = tmp_path / "script.txt"
    path.write_text("".join(ln + "\n" for ln in lines))
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")


def test_verdicts(checker, tmp_path):
    out = _run(checker, tmp_path, [f"verdict {T} {m} {p} {l} {s}" for T, m, p, l, s in VERDICTS])
    seen = set()
    for (T, m, p, l, s), ln in zip(VERDICTS, out):
        want = verdict(T, m, p, l, s)
        assert ln == f"verdict {want}", (T, m, p, l, s, ln)
        seen.add(want)
        if s <= 0:                       # the streaming form off, or a caller that knows four fields: what it was before
            assert want == (NOISELESS if not p else REFUSED_OFF if (T <= 0 or m != 0) else SERVED if l else REFUSED_PATH)
        if m == 1 and p:
            assert want == REFUSED_OFF   # mode 1 stays refused, whatever the new switch says
    assert seen == {NOISELESS, SERVED, REFUSED_OFF, REFUSED_PATH, SERVED_STREAM}


def test_chunk_planner(checker, tmp_path):
    """the program itself checks that the chunks cover every pair once and in order; the lines are the planner's numbers"""
    out = _run(checker, tmp_path, [f"plan {B} {T} {cap} 0 0" for B, T, cap in PLANS])
    want = [ln for B, T, cap in PLANS for ln in plan(B, T, cap)]
    assert out[:len(want)] == want
    assert plan(3, 3, 2)[-1] == "chunk 4 8 9 2 2 2 2" and plan(2, 4, 100)[0] == "plan 8 8 1" and plan(5, 3, 1)[0] == "plan 15 1 15"
    assert plan(40, 4096, 1 << 20)[0] == "plan 163840 65535 3"


# ---- the preconditions of the GPU parity cases ------------------------------------------------------------------------------
def test_preconditions_of_the_parity_cases():
    """over the checked realisations: a realisation without an error, an X or Y on the control in front of a CNOT, a Y,
    an error on both qubits of a two-qubit slot; an OP_PZ record at each of the three positions of a K = 3 backward
    group; two realisations of one circuit with different op counts; no draw on a threshold."""
    seen, pos, differ, margin = sng.preconditions()
    assert seen == {"none", "x_before_control", "y", "both"}
    assert pos == {0, 1, 2} and differ
    assert margin > 1e-12
    for n in sng.PARITY_N:
        case = sng.parity_case(n)
        for gates, th in case["circuits"]:
            assert gates[0].size <= 2 * sng.G_LONG and th.size <= 13
        assert case["ham"][2].size <= 12
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8} == {int(k) for g, _ in sng.parity_case(15)["circuits"] for k in g[0]}
    assert any(g[0].size == 2 * sng.G_SHORT for g, _ in sng.parity_case(14)["circuits"])
    assert sng.MAX_RESIDENT_16 < len(sng.parity_case(16)["circuits"]) * sng.T


def test_preconditions_of_the_table_case():
    """the Z-heavy table: at least ten Z errors over the checked realisations, every draw clear of its thresholds"""
    case = sng.parity_case(14)
    codes, margin = sng.parity_codes(case, w1=sng.W1, w2=sng.W2, p=sng.TABLE_P, seed=sng.TABLE_SEED)
    assert margin > 1e-12
    assert sum(int((c == 3).sum()) for per in codes.values() for c in per) >= 10
