"""CPU: the Hamiltonian layout planner (csrc/ham_layout.h) against the contract the energy kernels rely on.

tests/cpp/ham_layout_check.cpp plans the layout and the gradient tables of every shard of a Hamiltonian with the
library's own planner (a host-only header, built here with g++) and checks them EXACTLY - no tolerance - against values
recomputed from the term list and the definitions:

1. cover: over the shards rank = 0..world-1 every X-mask group is in exactly one shard, there either in the group list
   or in the unit list;
2. values: every table slot of the group list holds, bit for bit, the sign sum at the canonical pair representative it
   stands for (plain, class and diagonal groups; x' = M x, z' = M^-T z); every (unit, thread) address un-swizzles to a
   selector-0 representative, every unit value is the sign sum there or exactly 0.0 below the zero bound, and every
   pair above the bound is held exactly once;
3. shape: section order, zero padding to multiples of energy_pd(n) / kUnitUnroll, M^-1, mrow = S M, linearity of swz
   and where it must stay 0, mean <= mean0;
4. gradient tables: every entry the sign sum in the logical index, the complex flag exactly for groups with an
   imaginary coefficient.

The Hamiltonians are those of the GPU suites (tests/test_unit_addresses_gpu.py draws the fermionic ones in the same
order from the same generators), so what holds on a card - units > 0, a non-identity bank swizzle that lowers the
modelled conflicts of the bench Hamiltonian - is asserted here too."""
import os
import subprocess

import numpy as np
import pytest

import tensorrl_qas_amd as tq
from helpers import CASES, fermionic_hamiltonian, load_case, random_hamiltonian, random_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ham_layout_check.cpp")
WORLDS = (1, 2, 3)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("layout") / "ham_layout_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def _write_terms(path, n, xs, zs, coeff):
    """n, then ``x z cr ci`` per term: c i^{#Y} as the library splits it, hex floats (nothing is rounded in transit)."""
    with open(path, "w") as f:
        f.write(f"{n}\n")
        for x, z, w in zip(xs, zs, coeff):
            x, z, w = int(x), int(z), float(w)
            ny = bin(x & z).count("1") % 4
            cr, ci = ((w, 0.0), (0.0, w), (-w, 0.0), (0.0, -w))[ny]
            f.write(f"{x} {z} {cr.hex()} {ci.hex()}\n")


def _check(checker, tmp_path, n, ham, units_on=True, worlds=WORLDS):
    """Runs the check; returns {(world, rank): dict} of the shards' figures."""
    path = str(tmp_path / "terms.txt")
    _write_terms(path, n, *ham)
    r = subprocess.run([checker, path, "1" if units_on else "0"] + [str(w) for w in worlds],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("shard "):
            _, world, rank, groups, padding, units, swz, mean0, mean = line.split()
            out[(int(world), int(rank))] = dict(groups=int(groups), padding=int(padding), units=int(units),
                                                swz=int(swz, 16), mean0=float(mean0), mean=float(mean))
    assert sorted(out) == [(w, r) for w in worlds for r in range(w)]
    return out


@pytest.mark.parametrize("case", CASES)
def test_golden_hamiltonians(checker, tmp_path, case):
    d = load_case(case)
    xs, zs = tq.hamiltonian.masks_from_strings(d["paulis"], d["n"])
    lay = _check(checker, tmp_path, d["n"], (xs, zs, d["weights"]))
    if case == "H2O_8q":      # the shipped H2O Hamiltonian is held as units (smoke() asserts the same on a card)
        assert lay[(1, 0)]["units"] > 0


@pytest.mark.parametrize("n", [8, 9, 10, 11, 12, 13])
def test_fermionic_by_size(checker, tmp_path, n):
    rng = np.random.default_rng(7300 + n)
    random_state(n, rng)      # (the GPU test draws its initial state first)
    ham = fermionic_hamiltonian(n, 2 * n, 3 * n, rng, 3)
    lay = _check(checker, tmp_path, n, ham)
    assert lay[(1, 0)]["units"] > 0 and lay[(1, 0)]["units"] % 12 == 0


def test_bench_hamiltonian(checker, tmp_path):
    H = tq.hamiltonian.synthetic_lih12()
    lay = _check(checker, tmp_path, 12, (H.xmask, H.zmask, H.coeff))[(1, 0)]
    assert lay["units"] > 0 and lay["swz"] != 0 and 1.0 <= lay["mean"] < lay["mean0"], lay


def test_units_switched_off(checker, tmp_path):
    """VQE_UNITS=0: every group in the group list, no swizzle."""
    H = tq.hamiltonian.synthetic_lih12()
    for shard in _check(checker, tmp_path, 12, (H.xmask, H.zmask, H.coeff), units_on=False).values():
        assert shard["units"] == 0 and shard["swz"] == 0


@pytest.mark.parametrize("n", [6, 11])
def test_imaginary_section(checker, tmp_path, n):
    rng = np.random.default_rng(7600 + n)
    xs, zs, cs = random_hamiltonian(n, 60, rng, real=False)
    assert any(bin(int(x) & int(z)).count("1") % 2 for x, z in zip(xs, zs))
    _check(checker, tmp_path, n, (xs, zs, cs))


def test_streaming_path_terms(checker, tmp_path):
    """n = 14: no tables, no units - the term arrays of the shard's groups."""
    rng = np.random.default_rng(7614)
    lay = _check(checker, tmp_path, 14, random_hamiltonian(14, 80, rng, real=False))
    assert all(s["units"] == 0 and s["padding"] == 0 for s in lay.values())
