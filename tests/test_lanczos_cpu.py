"""CPU: the host logic of the device Lanczos solver (vqe_lanczos: csrc/lanczos_host.h) as far as it can be
held without a GPU.  tests/cpp/lanczos_host_check.cpp (a plain host program, built here with g++ -Wall -Werror) runs

(i)   lz_tridiag_extreme on tridiagonals generated here - the constant one, whose spectrum a + 2 b cos(k pi / (m + 1)) is
      known in closed form, and random ones - for m = 1, 2, 3, 64, 256 and both ends: the eigenvalue against
      numpy.linalg.eigvalsh of the same matrix within 1e-13 |T|, the vector by |T s - theta s| <= 1e-13 |T| and |s| = 1;
(ii)  lz_decide on hand-written histories, one per outcome, and the order of its tests;
(iii) lz_basis_capacity at its edges."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lanczos_host_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lanczos") / "lanczos_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _dense(alpha, beta):
    return np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1)


def _tridiag(checker, tmp_path, which, alpha, beta):
    path = str(tmp_path / "t.txt")
    with open(path, "w") as f:
        f.write(f"{which} {len(alpha)}\n{_hex(alpha)}\n{_hex(beta)}\n")
    r = subprocess.run([checker, "tridiag", path], capture_output=True, text=True, check=True)
    lines = r.stdout.splitlines()
    theta = float.fromhex(lines[0].split()[1])
    s = np.array([float.fromhex(v) for v in lines[1].split()[1:]])
    return theta, s


def _matrices(m):
    rng = np.random.default_rng(7100 + m)
    out = [("constant", np.full(m, 0.3), np.full(m - 1, -1.7)),
           ("constant+", np.full(m, -2.0), np.full(m - 1, 0.25))]
    for k in range(3):
        out.append((f"random{k}", rng.normal(size=m), rng.normal(size=m - 1)))
    # the shape of a converging Lanczos run: positive off-diagonals that decay by orders of magnitude
    out.append(("graded", rng.normal(size=m), np.abs(rng.normal(size=m - 1)) * np.logspace(0, -9, max(m - 1, 1))[:m - 1]))
    return out


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 3, 64, 256])
def test_tridiag_extreme_against_eigvalsh(checker, tmp_path, m, which):
    for name, alpha, beta in _matrices(m):
        T = _dense(alpha, beta)
        ev = np.linalg.eigvalsh(T)
        norm = max(abs(ev[0]), abs(ev[-1]))
        want = ev[-1] if which else ev[0]
        theta, s = _tridiag(checker, tmp_path, which, alpha, beta)
        assert s.size == m
        assert abs(theta - want) <= 1e-13 * norm, (name, theta, want)
        assert np.linalg.norm(T @ s - theta * s) <= 1e-13 * norm, (name, np.linalg.norm(T @ s - theta * s))
        assert abs(np.linalg.norm(s) - 1.0) <= 1e-14, name
        if name.startswith("constant"):
            a, b = alpha[0], (abs(beta[0]) if m > 1 else 0.0)
            exact = a + (2 * b if which else -2 * b) * np.cos(np.pi / (m + 1))
            assert abs(theta - exact) <= 1e-13 * norm, (name, theta, exact)


def _decide(checker, tmp_path, which, capacity, max_matvec, tol, steps, matvecs, broke, alpha, beta):
    assert len(alpha) == len(beta) == steps
    path = str(tmp_path / "d.txt")
    with open(path, "w") as f:
        f.write(f"{which} {capacity} {max_matvec} {float(tol).hex()} {steps} {matvecs} {broke}\n{_hex(alpha)}\n{_hex(beta)}\n")
    r = subprocess.run([checker, "decide", path], capture_output=True, text=True, check=True)
    w = r.stdout.split()
    return w[1], int(w[3]), float.fromhex(w[5])


def test_decide_one_history_per_outcome(checker, tmp_path):
    lo = lambda a, b, k: np.linalg.eigvalsh(_dense(a[:k], b[:k - 1]))[0]
    hi = lambda a, b, k: np.linalg.eigvalsh(_dense(a[:k], b[:k - 1]))[-1]
    # continue: three steps of a free chain, nothing small, room in the basis and in the budget
    a, b = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    d, dim, th = _decide(checker, tmp_path, 0, 8, 100, 1e-10, 3, 3, -1, a, b)
    assert (d, dim) == ("continue", 3) and abs(th - lo(a, b, 3)) <= 1e-14
    # converged: the last off-diagonal is far below tol - and convergence is seen before the spent budget and the full basis
    a, b = [1.0, 2.0, 3.0], [0.5, 0.5, 1e-13]
    d, dim, th = _decide(checker, tmp_path, 0, 3, 3, 1e-10, 3, 3, -1, a, b)
    assert (d, dim) == ("converged", 3) and abs(th - lo(a, b, 3)) <= 1e-14
    # converged by a small last component of the Ritz vector, beta itself of order one: the highest end of a graded T
    a, b = [10.0, 0.0, 0.0, 0.0], [1e-4, 1e-4, 1e-4, 1.0]
    d, dim, th = _decide(checker, tmp_path, 1, 8, 100, 1e-10, 4, 4, -1, a, b)
    assert (d, dim) == ("converged", 4) and abs(th - hi(a, b, 4)) <= 1e-14
    # ... while the lowest end of the same history is not converged: |beta s_last| ~ 0.5
    d, dim, th = _decide(checker, tmp_path, 0, 8, 100, 1e-10, 4, 4, -1, a, b)
    assert (d, dim) == ("continue", 4)
    # restart: the basis is full, not converged, budget left
    a, b = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    d, dim, th = _decide(checker, tmp_path, 0, 3, 100, 1e-10, 3, 40, -1, a, b)
    assert (d, dim) == ("restart", 3)
    # budget: it is seen before the full basis
    d, dim, th = _decide(checker, tmp_path, 0, 3, 40, 1e-10, 3, 40, -1, a, b)
    assert (d, dim) == ("budget", 3) and abs(th - lo(a, b, 3)) <= 1e-14
    d, dim, th = _decide(checker, tmp_path, 0, 8, 5, 1e-10, 3, 5, -1, a, b)
    assert (d, dim) == ("budget", 3)
    # breakdown at step 1 of the cycle: the pair of T_2, whatever the later (never computed) entries hold
    a, b = [1.0, -1.0, 123.0], [0.5, 1e-17, 456.0]
    d, dim, th = _decide(checker, tmp_path, 0, 8, 100, 1e-10, 3, 2, 1, a, b)
    assert (d, dim) == ("breakdown", 2) and abs(th - lo(a, b, 2)) <= 1e-14
    # breakdown at step 0: the start vector is an eigenvector, theta = alpha_0, for either end
    for which in (0, 1):
        d, dim, th = _decide(checker, tmp_path, which, 8, 100, 1e-10, 1, 1, 0, [0.75], [0.0])
        assert (d, dim, th) == ("breakdown", 1, 0.75)


def _capacity(checker, budget, n, max_basis):
    r = subprocess.run([checker, "capacity", str(budget), str(n), str(max_basis)], capture_output=True, text=True, check=True)
    return int(r.stdout)


def test_basis_capacity_edges(checker):
    vec = lambda n: 16 << n
    assert _capacity(checker, 10 ** 12, 3, 128) == 8             # 2^n < max_basis
    assert _capacity(checker, 10 ** 12, 1, 128) == 2
    assert _capacity(checker, 10 ** 12, 10, 128) == 128          # max_basis decides
    assert _capacity(checker, 10 ** 12, 10, 2) == 2
    assert _capacity(checker, (5 + 3) * vec(10), 10, 128) == 5   # a budget that holds exactly 5 vectors beside the 3 work vectors
    assert _capacity(checker, (5 + 3) * vec(10) - 1, 10, 128) == 4
    assert _capacity(checker, (2 + 3) * vec(10), 10, 128) == 2   # the least that runs
    assert _capacity(checker, (2 + 3) * vec(10) - 1, 10, 128) == 1      # below 2: the call answers VQE_ENOMEM
    assert _capacity(checker, 3 * vec(10), 10, 128) == 0
    assert _capacity(checker, 0, 10, 128) == 0
    assert _capacity(checker, 10 * vec(30), 30, 128) == 7        # 16 GiB vectors: the products do not wrap


def test_abi_has_the_entry_points():
    from tensorrl_qas_amd import _lib
    lib = _lib.load()
    o = _lib.LanczosOpts()
    assert lib.vqe_lanczos_default_opts(C.byref(o)) == 0
    assert (o.which, o.max_basis, o.max_matvec, o.check_every, o.start_from_init, o.tol, o.seed) == (0, 128, 2000, 8, 0, 1e-10, 1)
    assert lib.vqe_lanczos_default_opts(None) == -22             # VQE_EINVAL
    ev, info = C.c_double(), (C.c_double * 4)()
    assert lib.vqe_lanczos(None, None, C.byref(ev), None, info) == -22
    assert lib.vqe_lanczos_dev(None, None, C.byref(ev), None, info) == -22
