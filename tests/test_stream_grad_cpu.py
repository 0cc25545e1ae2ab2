"""The opt-in switch of the streaming-path gradient is part of the C ABI and of the ctypes signature table."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vqe_set_stream_grad_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "vqe_hip.h")).read()
    assert re.search(r"\bint\s+vqe_set_stream_grad\s*\(\s*vqe_t\s*\*\s*h\s*,\s*int\s+enable\s*\)\s*;", header)
    from tensorrl_qas_amd import _lib
    assert _lib.SIGNATURES["vqe_set_stream_grad"] == (C.c_int, [_lib.vp, C.c_int])
