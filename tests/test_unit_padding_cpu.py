"""CPU: the look-ahead trips behind the unit arrays (csrc/ham_layout.h: unit_arrays).

The unit loop of the energy step accumulates one trip of 4 units while it prefetches the tables and addresses of the
trip two ahead and the record of the next one.  The host appends two zero trips to the arrays it uploads, so that the
loop's offsets step by constants up to the last trip and nothing is clamped.  tests/cpp/unit_padding_check.cpp plans
a Hamiltonian with the library's own planner (the host-only header, built here with g++, the route of
tests/test_ham_layout_cpu.py) and checks exactly:

1. the arrays hold the accumulated trips - the layout's units, unchanged bit for bit - plus two look-ahead trips;
2. the look-ahead trips are zero records, +0.0 tables and addresses inside the state; the loop's last requests end
   inside the arrays;
3. n_units (the loop bound) and the bank-swizzle score are what they are without the padding.

The Hamiltonians are number-conserving sums whose only off-diagonal terms are k double-excitation octets: each octet is
one X-mask group that acts on one occupation pattern in eight and is held as exactly one unit at 8, 10 and 12 qubits,
so the unit count before padding is k.  k = 1, 4, 5, 11, 12, 13 covers every residue of the trip (4) and of the
turn (12); tests/test_hot_loop_addresses_gpu.py runs the same Hamiltonians on a card."""
import os
import subprocess

import numpy as np
import pytest

from helpers import fermionic_hamiltonian, random_hamiltonian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "unit_padding_check.cpp")
UNIT_COUNTS = (1, 4, 5, 11, 12, 13)


def octet_hamiltonian(n, k, seed):
    """Identity + Z + ZZ terms and k double-excitation octets on n qubits: k units."""
    return fermionic_hamiltonian(n, 0, k, np.random.default_rng(seed), 0)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("unitpad") / "unit_padding_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def _write_terms(path, n, xs, zs, coeff):
    """n, then ``x z cr ci`` per term: c i^{#Y} as the library splits it, hex floats (the format of ham_layout_check)."""
    with open(path, "w") as f:
        f.write(f"{n}\n")
        for x, z, w in zip(xs, zs, coeff):
            x, z, w = int(x), int(z), float(w)
            ny = bin(x & z).count("1") % 4
            cr, ci = ((w, 0.0), (0.0, w), (-w, 0.0), (0.0, -w))[ny]
            f.write(f"{x} {z} {cr.hex()} {ci.hex()}\n")


def _check(checker, tmp_path, n, ham, want):
    path = str(tmp_path / "terms.txt")
    _write_terms(path, n, *ham)
    r = subprocess.run([checker, path, str(want)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("units ")][0].split()
    return int(line[1]), int(line[2]), int(line[3])


# LT = 6 (one wave) at 8 qubits, LT = 8 at 10 and 12 (the sizes of the GPU test)
@pytest.mark.parametrize("n", [8, 10, 12])
@pytest.mark.parametrize("k", UNIT_COUNTS)
def test_lookahead_trips(checker, tmp_path, n, k):
    real, n_units, total = _check(checker, tmp_path, n, octet_hamiltonian(n, k, 8100 + 16 * n + k), k)
    assert real == k
    assert n_units == 12 * ((k + 11) // 12)       # whole turns, as before
    assert total == n_units + 8                   # plus two trips of four units


def test_no_units_no_lookahead(checker, tmp_path):
    """A dense random Hamiltonian has no units: nothing is appended (the loop returns before its first request)."""
    rng = np.random.default_rng(8099)
    assert _check(checker, tmp_path, 10, random_hamiltonian(10, 40, rng), 0) == (0, 0, 0)
