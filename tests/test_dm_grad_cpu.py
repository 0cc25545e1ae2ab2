"""CPU: the adjoint gradient of the batched exact channel mode (vqe_set_dm_grad: csrc/vqe_dm_grad.h) as far
as it can be held without a GPU.  tests/cpp/dm_grad_check.cpp (a plain host program, built here with g++) holds

(i)   the derivative chain of csrc/dm_build.h (the member list with the generator behind a rotation member, what
      k_dmg_contract runs) against the exact shift (S(theta + pi/2) - S(theta - pi/2)) / 2 of dm_fill_blocks, per entry,
      <= 1e-14 of the block's largest entry, every rotation with an angle of its own: n = 2, 3, 5, 8, 12 and the
      high-window circuit of test_dm_plan_cpu.py at (p1, p2) = (0, 0), (1, 1), (0.01, 0.05);
(ii)  the whole formula - states kept, Lambda_L = conj(h), M_l, the contraction, Lambda_{l-1} = S_l^+ Lambda_l - as a
      plain host loop at n = 2, 3, 4 against the parameter shift of the host energy, <= 1e-12: the conjugations and the
      sign of the generator;
(iii) the memory rule dm_grad_resident (csrc/dm_host.h) and the split of a level into partial sums, as pure functions."""
import os
import subprocess

import numpy as np
import pytest

from dm_batch_cases import gate_list, mixed_batch, noisy
from helpers import random_gates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dm_grad_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dmgrad") / "dm_grad_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def _run(checker, tmp_path, what, n, circuits, p1=0.07, p2=0.11):
    path = str(tmp_path / "circuits.txt")
    with open(path, "w") as f:
        f.write(f"{n} {float(p1).hex()} {float(p2).hex()} {len(circuits)}\n")
        for kind, q0, q1, pidx, th in circuits:
            f.write(f"{len(kind)} {len(th)}\n")
            for g in zip(kind, q0, q1, pidx):
                f.write(" ".join(str(int(v)) for v in g) + "\n")
            f.write(" ".join(float(t).hex() for t in th) + "\n")
    r = subprocess.run([checker, what, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    return {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.strip()}


@pytest.mark.parametrize("n", [2, 3, 5, 8, 12])
def test_derivative_chain_against_the_exact_shift(checker, tmp_path, n):
    rng = np.random.default_rng(5100 + n)
    circuits = [noisy(random_gates(n, G, rng)) for G in (0, 1, 7, 40)] + mixed_batch(n, 24, rng)
    circuits.append(noisy(random_gates(n, 30, rng, p_cnot=0.15)))      # long member lists: several rotations per block
    out = _run(checker, tmp_path, "chain", n, circuits)
    assert int(out["members"][0]) >= 40 and float(out["chain"][0]) <= 1e-14


@pytest.mark.parametrize("p1,p2", [(0.0, 0.0), (1.0, 1.0), (0.01, 0.05)])
def test_derivative_chain_high_window_and_strong_channels(checker, tmp_path, p1, p2):
    """The n = 12 circuit of test_high_window_bits_and_strong_channels, with and without its channels."""
    circ = gate_list([(0, 4, 5, None), (1, 10, -1, 0.7), (0, 10, 11, None), (3, 11, -1, -1.1), (0, 11, 0, None), (2, 0, -1, 0.2),
                      (1, 5, -1, 2.0), (0, 0, 11, None)])
    out = _run(checker, tmp_path, "chain", 12, [noisy(circ), circ], p1, p2)
    assert int(out["members"][0]) == 8 and float(out["chain"][0]) <= 1e-14


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("p1,p2", [(0.01, 0.05), (0.75, 0.9375), (0.0, 0.0)])
def test_whole_formula_on_the_host(checker, tmp_path, n, p1, p2):
    rng = np.random.default_rng(5200 + n)
    circuits = [noisy(random_gates(n, G, rng)) for G in (0, 1, 9)] + mixed_batch(n, 12, rng)
    # channels behind only some gates: at the singular strengths the gradient is not identically zero
    base = random_gates(n, 10, rng, p_cnot=0.3)
    full = noisy(base)
    keep = [i for i in range(len(full[0])) if full[0][i] < 4 or (i // 2) % 3 == 0]
    circuits.append(tuple(np.asarray(v)[keep] for v in full[:4]) + (full[4],))
    out = _run(checker, tmp_path, "formula", n, circuits, p1, p2)
    assert int(out["parameters"][0]) >= 10 and float(out["formula"][0]) <= 1e-12


def _resident(checker, budget, n, levels, batch):
    r = subprocess.run([checker, "resident", str(budget), str(n), str(levels), str(batch)], capture_output=True, text=True, check=True)
    return int(r.stdout)


def test_memory_rule(checker):
    dm = lambda n: 16 * 4 ** n
    # levels + 2 density matrices per resident circuit
    assert _resident(checker, 12 * dm(5), 5, 10, 8) == 1
    assert _resident(checker, 12 * dm(5) - 1, 5, 10, 8) == 0          # less than one circuit: the call answers VQE_ENOMEM
    assert _resident(checker, 0, 5, 10, 8) == 0
    assert _resident(checker, 1 * dm(5), 5, 0, 8) == 0                # even a circuit without gates keeps rho_0 and Lambda
    assert _resident(checker, 2 * dm(5), 5, 0, 8) == 1
    assert _resident(checker, 36 * dm(5) + 5, 5, 10, 8) == 3          # forced below the batch by the kept states
    assert _resident(checker, 1000 * dm(5), 5, 10, 8) == 8            # more than the batch
    assert _resident(checker, 12 * dm(13), 13, 10, 4) == 1            # 1 GiB matrices: the product does not wrap
    assert _resident(checker, 2 * 70000 * dm(2), 2, 0, 100000) == 65535      # the y extent of a grid
    assert _resident(checker, 2 * 70000 * dm(2), 2, 0, 65534) == 65534


def test_partial_sums_are_a_function_of_n_alone(checker):
    for n in range(2, 14):
        r = subprocess.run([checker, "partials", str(n)], capture_output=True, text=True, check=True)
        tiles, tpp, parts = (int(v) for v in r.stdout.split())
        assert tiles == max(1, 4 ** n // 256) and tpp >= 4 and 1 <= parts <= 256
        assert (parts - 1) * tpp < tiles <= parts * tpp or (tiles < tpp and parts == 1)


def test_abi_has_the_switch():
    from tensorrl_qas_amd import _lib
    assert _lib.SIGNATURES["vqe_set_dm_grad"] == _lib.SIGNATURES["vqe_set_stream_grad"]
    lib = _lib.load()
    assert lib.vqe_set_dm_grad(None, 1) == -22           # VQE_EINVAL for a NULL handle
