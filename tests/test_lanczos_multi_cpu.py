"""CPU: the host logic of vqe_lanczos_multi (csrc/lanczos_host.h) as far as it can be held without a GPU.
tests/cpp/lanczos_multi_host_check.cpp (a plain host program, built here with g++ -Wall -Werror) runs

(i)   lz_sym_eig, the dense symmetric eigensolver of the thick restart, on the matrices a restart produces - a diagonal
      bordered by one row and column, tridiagonal after it - up to order 256: eigenvalues against numpy.linalg.eigvalsh
      within 1e-13 |T| (the bound lz_tridiag_extreme is held to).  Vectors: the method (Householder, implicit QL) is
      backward stable, its pairs are exact for T + E with |E| a small multiple of n eps |T|; the residual of every pair
      and the defect of Z^T Z are held to max(1e-13, 4 n eps) |T| resp. max(1e-13, 4 n eps) - 2.3e-13 at n = 256;
(ii)  lz_keep_count and the storage rule (slots, capacity per stage, the VQE_ENOMEM condition);
(iii) the LzMulti state machine driving plain-loop vector arithmetic on a dense Hermitian 32 x 32 matrix whose lowest
      level is 3-fold, active capacity 4 and 8 (and 2: no room for a thick restart), six pairs, both ends: eigenvalues
      within 1e-9 of eigvalsh - with multiplicity, since the sorted spectra are compared entry by entry -, true residuals
      <= 10 tol max(1, |theta|) and |Y^H Y - I|max <= tol (the bounds of the GPU tests)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lanczos_multi_host_check.cpp")
EPS = np.finfo(np.float64).eps
TOL = 1e-10


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lanczos_multi") / "lanczos_multi_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"),
                    SRC, "-o", str(exe)], check=True)
    return str(exe)


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, np.float64).reshape(-1))


def _unhex(words):
    return np.array([float.fromhex(v) for v in words])


def _symeig(checker, tmp_path, T):
    n = T.shape[0]
    path = str(tmp_path / "a.txt")
    with open(path, "w") as f:
        f.write(f"{n}\n{_hex(T)}\n")
    r = subprocess.run([checker, "symeig", path], capture_output=True, text=True, check=True)
    lines = r.stdout.splitlines()
    return _unhex(lines[0].split()[1:]), _unhex(lines[1].split()[1:]).reshape(n, n)


def _restart_matrix(n, r, rng, graded=False):
    """diag(theta_0 .. theta_{r-1}) bordered by b in row / column r, tridiagonal from r on"""
    T = np.zeros((n, n))
    T[np.arange(n), np.arange(n)] = rng.normal(size=n)
    r = min(r, n - 1)
    for i in range(r):
        T[i, r] = T[r, i] = rng.normal() * (10.0 ** -rng.uniform(0, 9) if graded else 1.0)
    for j in range(r, n - 1):
        T[j, j + 1] = T[j + 1, j] = abs(rng.normal()) * (10.0 ** (-9.0 * j / n) if graded else 1.0)
    return T


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 64, 256])
def test_sym_eig_against_eigvalsh(checker, tmp_path, n):
    rng = np.random.default_rng(7300 + n)
    cases = [("tridiagonal", _restart_matrix(n, 0, rng)), ("arrow1", _restart_matrix(n, 1, rng)),
             ("arrow-half", _restart_matrix(n, n // 2, rng)), ("arrow-all", _restart_matrix(n, n - 1, rng)),
             ("arrow-graded", _restart_matrix(n, n // 2, rng, graded=True)),
             ("degenerate", np.diag(np.repeat(rng.normal(size=(n + 2) // 3), 3)[:n])),
             ("full", (lambda a: a + a.T)(rng.normal(size=(n, n))))]
    slack = max(1e-13, 4 * n * EPS)
    for name, T in cases:
        ev = np.linalg.eigvalsh(T)
        norm = max(abs(ev[0]), abs(ev[-1]))
        w, Z = _symeig(checker, tmp_path, T)
        assert np.all(np.diff(w) >= 0.0), name
        assert np.max(np.abs(w - ev)) <= 1e-13 * norm, (name, np.max(np.abs(w - ev)) / norm)
        res = np.max(np.linalg.norm(T @ Z - Z * w, axis=0))
        assert res <= slack * norm, (name, res / norm)
        assert np.max(np.abs(Z.T @ Z - np.eye(n))) <= slack, name


def _keep(checker, capacity, keep):
    return int(subprocess.run([checker, "keep", str(capacity), str(keep)], capture_output=True, text=True, check=True).stdout)


def test_keep_count(checker):
    # below 3 active vectors there is no room for (Ritz vector, residual vector, one new step): an explicit restart
    assert [_keep(checker, c, 0) for c in (1, 2)] == [0, 0] and _keep(checker, 2, 1) == 0
    # the library's rule: half the basis, within 1 .. capacity - 2
    assert [_keep(checker, c, 0) for c in (3, 4, 5, 8, 16, 128)] == [1, 2, 2, 4, 8, 64]
    # the caller's count, clamped to what a stage's basis allows
    assert _keep(checker, 8, 1) == 1 and _keep(checker, 8, 5) == 5 and _keep(checker, 8, 6) == 6
    assert _keep(checker, 8, 7) == 6 and _keep(checker, 8, 100) == 6 and _keep(checker, 3, 5) == 1
    for c in range(3, 40):
        for k in range(0, 45):
            assert 1 <= _keep(checker, c, k) <= c - 2


def _slots(checker, budget, n, max_basis, n_eig):
    r = subprocess.run([checker, "slots", str(budget), str(n), str(max_basis), str(n_eig)], capture_output=True, text=True, check=True)
    w = [int(v) for v in r.stdout.split()]
    return w[0], bool(w[1]), w[2:]


def test_storage_rule(checker):
    vec = lambda n: 16 << n
    big = 10 ** 13
    # memory to spare: max_basis + n_eig - 1 slots, every stage has max_basis active vectors
    assert _slots(checker, big, 10, 8, 6) == (13, True, [8] * 6)
    # 2^n decides: the full spectrum of 3 qubits - the active basis shrinks with the complement, the last stage has one vector
    assert _slots(checker, big, 3, 128, 8) == (8, True, [8, 7, 6, 5, 4, 3, 2, 1])
    assert _slots(checker, big, 1, 128, 2) == (2, True, [2, 1])
    assert _slots(checker, big, 2, 2, 4) == (4, True, [2, 2, 2, 1])
    # the budget decides: 3 work vectors + 7 slots; locked vectors take their slots from the active basis
    assert _slots(checker, 10 * vec(10), 10, 8, 6) == (7, True, [7, 6, 5, 4, 3, 2])
    # ... and one slot less leaves the last stage a single active vector of a large complement: VQE_ENOMEM
    assert _slots(checker, 10 * vec(10) - 1, 10, 8, 6) == (6, False, [6, 5, 4, 3, 2, 1])
    assert _slots(checker, 3 * vec(10), 10, 8, 1) == (0, False, [0])
    assert _slots(checker, 5 * vec(10), 10, 8, 1) == (2, True, [2])
    assert _slots(checker, 10 * vec(30), 30, 128, 6) == (7, True, [7, 6, 5, 4, 3, 2])      # 16 GiB vectors: nothing wraps


def _run(checker, tmp_path, H, n_eig, max_basis, which=0, max_matvec=100000, check_every=8, keep=0, tol=TOL, seed=1, slots=None):
    dim = H.shape[0]
    n = dim.bit_length() - 1
    slots = min(max_basis + n_eig - 1, dim) if slots is None else slots
    path = str(tmp_path / "h.txt")
    Hc = np.ascontiguousarray(H, np.complex128)
    with open(path, "w") as f:
        f.write(f"{n} {which} {n_eig} {max_basis} {max_matvec} {check_every} {keep} {float(tol).hex()} {seed} {slots}\n")
        f.write(_hex(Hc.view(np.float64)) + "\n")
    r = subprocess.run([checker, "run", path], capture_output=True, text=True, check=True)
    lines = r.stdout.splitlines()
    status, matvecs, restarts, pairs = (int(v) for v in lines[0].split()[1:])
    theta, resid = _unhex(lines[1].split()[1:]), _unhex(lines[2].split()[1:])
    Y = np.array([_unhex(l.split()[2:]).view(np.complex128) for l in lines[3:3 + pairs]]).reshape(pairs, dim)
    return dict(status=status, matvecs=matvecs, restarts=restarts, pairs=pairs, theta=theta, resid=resid, Y=Y)


@pytest.fixture(scope="module")
def threefold():
    """A dense complex Hermitian 32 x 32 matrix with the spectrum -2 (x3), -1.5 (x2), -1, 20 more distinct values in
    (0, 3), 4 (x2) and 5 (x4)."""
    rng = np.random.default_rng(7400)
    w = np.concatenate([[-2.0] * 3, [-1.5] * 2, [-1.0], np.sort(rng.uniform(0.0, 3.0, 20)), [4.0] * 2, [5.0] * 4])
    Q, _ = np.linalg.qr(rng.normal(size=(32, 32)) + 1j * rng.normal(size=(32, 32)))
    H = (Q * w) @ Q.conj().T
    H = 0.5 * (H + H.conj().T)
    return H, np.linalg.eigvalsh(H)


def _check(out, H, ev, which, k, tol=TOL):
    want = ev[::-1][:k] if which else ev[:k]
    assert out["pairs"] == k and out["status"] in (0, 1)
    print(f"theta - eig = {np.max(np.abs(out['theta'] - want)):.3e}  matvecs = {out['matvecs']}  restarts = {out['restarts']}")
    assert np.max(np.abs(out["theta"] - want)) <= 1e-9
    Y = out["Y"]
    for e in range(k):
        host_r = np.linalg.norm(H @ Y[e] - out["theta"][e] * Y[e])
        R = 10.0 * tol * max(1.0, abs(out["theta"][e]))
        assert host_r <= R and out["resid"][e] <= R
    assert np.max(np.abs(Y.conj() @ Y.T - np.eye(k))) <= tol


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("capacity", [2, 4, 8])
def test_state_machine_on_a_threefold_level(checker, tmp_path, threefold, capacity, which):
    H, ev = threefold
    out = _run(checker, tmp_path, H, 6, capacity, which=which)
    _check(out, H, ev, which, 6)
    assert out["restarts"] >= 1


def test_state_machine_full_spectrum_and_budget(checker, tmp_path, threefold):
    H, ev = threefold
    # every pair of a 3-qubit matrix: the last stages end in a breakdown or a one-dimensional complement
    rng = np.random.default_rng(7401)
    A = rng.normal(size=(8, 8)) + 1j * rng.normal(size=(8, 8))
    A = A + A.conj().T
    out = _run(checker, tmp_path, A, 8, 128)
    _check(out, A, np.linalg.eigvalsh(A), 0, 8)
    assert out["status"] == 1 and out["restarts"] == 0
    # a budget that ends inside stage 2: two pairs, status 2 - and what was found is what the unbounded run found
    two = _run(checker, tmp_path, H, 2, 8)
    three = _run(checker, tmp_path, H, 3, 8)
    assert two["matvecs"] + 1 < three["matvecs"]
    cut = _run(checker, tmp_path, H, 3, 8, max_matvec=two["matvecs"] + 1)
    assert (cut["status"], cut["pairs"], cut["matvecs"]) == (2, 2, two["matvecs"] + 1)
    assert np.array_equal(cut["theta"], two["theta"]) and np.array_equal(cut["Y"], two["Y"])
    # the keep option changes the path, not the answer
    for keep in (1, 3, 6):
        _check(_run(checker, tmp_path, H, 6, 8, keep=keep), H, ev, 0, 6)


def test_abi_has_the_entry_points():
    from tensorrl_qas_amd import _lib
    lib = _lib.load()
    o = _lib.LanczosMultiOpts()
    assert lib.vqe_lanczos_multi_default_opts(C.byref(o)) == 0
    assert (o.which, o.n_eig, o.max_basis, o.max_matvec, o.check_every, o.keep, o.tol, o.seed) == (0, 1, 128, 2000, 8, 0, 1e-10, 1)
    assert lib.vqe_lanczos_multi_default_opts(None) == -22             # VQE_EINVAL
    ev, res, info = (C.c_double * 1)(), (C.c_double * 1)(), (C.c_double * 5)()
    assert lib.vqe_lanczos_multi(None, None, ev, None, res, info) == -22
    assert lib.vqe_lanczos_multi_dev(None, None, ev, None, res, info) == -22


def test_level_structure():
    from tensorrl_qas_amd import hamiltonian
    v = [-37.0862980001, -37.0862979999, -37.086298, -36.9, -36.5, -36.5 + 5e-9]
    assert hamiltonian.level_structure(v, 1e-8) == [(pytest.approx(-37.086298, abs=1e-9), 3), (-36.9, 1),
                                                    (pytest.approx(-36.5, abs=1e-8), 2)]
    assert hamiltonian.level_structure(v[::-1], 1e-8)[0][1] == 2      # descending values (which = "max") keep their order
    assert hamiltonian.level_structure([], 1e-8) == []
    assert hamiltonian.level_structure([1.0, 1.0 + 2e-8], 1e-8) == [(1.0, 1), (1.0 + 2e-8, 1)]
