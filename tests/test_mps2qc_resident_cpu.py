"""CPU: the host logic of the resident streaming fit (csrc/mps2qc_resident.h) as far as it can be held
without a GPU.  tests/cpp/stream_fit_host_check.cpp (a plain host program, built here with g++ -Wall -Werror) prints

(i)   sfd_bitrev - the index function k_sfd_load_target gathers through - for every index at n = 1 .. 12 and for
      sampled indices at n = 20 and 26, compared with the reversal of the n-character binary string;
(ii)  the option check: the defaults, and one case per refusal;
(iii) the buffer sizes at n = 2, 10, 11, 20 and 26 against the formulas written out below (no 32-bit wrap at 26 qubits
      with batch 4 and 50 gates);
(iv)  the number of step sequences the host loop enqueues at most, for max_iter and check_every around each other."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stream_fit_host_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_fit") / "stream_fit_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def _run(checker, *args):
    return subprocess.run([checker, *map(str, args)], capture_output=True, text=True, check=True).stdout


def _rev(i, n):
    return int(format(i, f"0{n}b")[::-1], 2)


@pytest.mark.parametrize("n", range(1, 13))
def test_bitrev_every_index(checker, n):
    got = [int(v) for v in _run(checker, "bitrev_all", n).split()]
    assert got == [_rev(i, n) for i in range(1 << n)]
    assert sorted(got) == list(range(1 << n))                       # a permutation ...
    assert [got[g] for g in got] == list(range(1 << n))             # ... that is its own inverse


@pytest.mark.parametrize("n", [20, 26])
def test_bitrev_sampled_indices(checker, n):
    rng = np.random.default_rng(n)
    idx = [0, 1, 2, (1 << n) - 1, (1 << n) - 2, 1 << (n - 1), (1 << (n - 1)) + 1] + [int(v) for v in rng.integers(0, 1 << n, 200)]
    got = [int(v) for v in _run(checker, "bitrev", n, *idx).split()]
    assert got == [_rev(i, n) for i in idx]


def test_option_check(checker):
    assert _run(checker, "defaults").split() == ["0", "0", "8", "-1"]
    for ok in ((0, 0, 8, -1), (1, 1, 1, 0), (0, 1, 1 << 20, 1), (1, 0, 64, -1)):
        assert _run(checker, "opts", *ok) == "ok\n", ok
    refusals = {(2, 0, 8, -1): "target_on_device", (-1, 0, 8, -1): "target_on_device",
                (0, 2, 8, -1): "target_little_endian", (0, -1, 8, -1): "target_little_endian",
                (0, 0, 0, -1): "check_every", (0, 0, -5, -1): "check_every",
                (0, 0, 8, 2): "use_graph", (0, 0, 8, -2): "use_graph"}
    for o, word in refusals.items():
        out = _run(checker, "opts", *o)
        assert out.startswith("refused mps2qc_fit_brickwork_resident: ") and word in out, (o, out)


@pytest.mark.parametrize("n,G,batch", [(2, 1, 1), (2, 3, 2), (10, 18, 2), (11, 10, 3), (20, 19, 2), (26, 50, 4)])
def test_buffer_sizes(checker, n, G, batch):
    blocks_amp, blocks_vec, states, env_part, ov_part = (int(v) for v in _run(checker, "sizes", n, G, batch).split())
    threads = 256
    dim = 1 << n
    assert blocks_amp == -(-dim // threads)                          # one thread per amplitude
    assert blocks_vec == -(-(dim // 4) // threads)                   # one thread per 4-vector
    assert states == batch * dim
    assert env_part == batch * G * blocks_vec * 16                   # [B][G][block][16]
    assert ov_part == batch * blocks_amp                             # [B][block]
    if n == 2:
        assert (blocks_amp, blocks_vec) == (1, 1)
    if n == 10:
        assert blocks_vec == 1 and blocks_amp == 4                   # exactly one block of 4-vectors
    if n == 11:
        assert blocks_vec == 2
    if n == 26:
        assert blocks_vec * 16 * 16 == 16 << 20                      # 16 MiB per gate and fit
        assert env_part == 4 * 50 * 65536 * 16 and env_part * 16 > 1 << 31      # 3.1 GiB: no int holds the byte count


def test_steps_enqueued(checker):
    for max_iter, every, want in ((1, 1, 1), (10, 4, 12), (10, 16, 16), (16, 16, 16), (17, 16, 32), (10, 1, 10),
                                  (2 ** 31 - 1, 2 ** 30, 2 ** 31)):
        assert int(_run(checker, "steps", max_iter, every)) == want, (max_iter, every)


def test_abi_has_the_entry_points():
    import ctypes as C
    from tensorrl_qas_amd import _lib
    lib = _lib.load_mps2qc()
    o = _lib.ResidentOpts()
    assert lib.mps2qc_resident_default_opts(C.byref(o)) == 0
    assert (o.target_on_device, o.target_little_endian, o.check_every, o.use_graph) == (0, 0, 8, -1)
    assert lib.mps2qc_resident_default_opts(None) == -22 and lib.mps2qc_last_error() != b""
    assert hasattr(lib, "mps2qc_fit_brickwork_resident")
