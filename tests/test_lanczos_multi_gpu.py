"""GPU: several eigenpairs by the device Lanczos (vqe_lanczos_multi / vqe_lanczos_multi_dev, VQEEngine.lanczos_multi;
thick restart and locking by deflation, csrc/vqe_lanczos.h, csrc/lanczos_host.h).

Bounds, none of them fitted: eigenvalues within 1e-9 of the reference spectrum (the tolerance of test_oracle.py); true
residuals, from the device and recomputed on the host, <= R = 10 tol max(1, |theta|) (test_lanczos_gpu.py); the
orthonormality defect |Y^H Y - I|max <= tol = 1e-10 - a defect above the tolerance the pairs were converged to is a
failure; and for every vector the Davis-Kahan inequality |(I - P_c) y| <= r_host / delta, P_c the projector on the
reference eigenspace of its level (reference eigenvalues within 1e-8 of each other), delta the distance from theta to
the nearest reference eigenvalue outside the level.

Measured on an MI355X (the figures the tests print): see the docstrings of the tests."""
import ctypes as C

import numpy as np
import pytest

import vqe_oracle as vo
from helpers import CASES, load_case, random_gates, with_noise_gates

pytestmark = pytest.mark.gpu

TOL = 1e-10           # the library's default
ESTATE, EINVAL = -1, -22


def bound(theta, tol=TOL):
    return 10.0 * tol * max(1.0, abs(theta))


def _engine(n, xs, zs, cs):
    import tensorrl_qas_amd as tq
    eng = tq.VQEEngine(n, 0)
    eng.set_hamiltonian(xs, zs, cs)
    return eng


@pytest.fixture(scope="module")
def problems():
    """name -> dict(n, xs, zs, cs, dense, eigvals, w, U): the fixtures of helpers.CASES with the oracle's dense matrix and
    its eigh (computed once, never changed).  The reference spectrum `eigvals` is w of that eigh: the molecular fixtures
    store the same full spectrum (held here to 1e-9), heisenberg_5q stores its distinct levels only."""
    import tensorrl_qas_amd as tq
    out = {}
    for case in CASES:
        d = load_case(case)
        xs, zs = tq.hamiltonian.masks_from_strings(d["paulis"], d["n"])
        p = dict(n=d["n"], xs=xs, zs=zs, cs=d["weights"], dense=vo.pauli_dense(d["paulis"], d["weights"], d["n"]),
                 stored=np.sort(np.asarray(d["eigvals"], np.float64)))
        p["w"], p["U"] = np.linalg.eigh(p["dense"])
        p["eigvals"] = p["w"]
        if p["stored"].size == p["w"].size:
            assert np.max(np.abs(p["stored"] - p["w"])) <= 1e-9
        assert abs(p["stored"][0] - p["w"][0]) <= 1e-9 and abs(p["stored"][-1] - p["w"][-1]) <= 1e-9
        out[case] = p
    return out


def _check(p, which, k, vals, vecs, info, tol=TOL, status=(0, 1)):
    """the bounds of test 1 for the k returned pairs (status 1: a stage exhausted its Krylov space - heisenberg_5q has 12
    distinct eigenvalues in 32 dimensions - and its pair is exact in it; the bounds are the same)"""
    ref = p["eigvals"][::-1] if which == "max" else p["eigvals"]
    w, U = p["w"], p["U"]
    assert info["pairs"] == k and vals.shape == (k,) and vecs.shape == (k, 1 << p["n"]) and info["status"] in status
    assert np.all(np.diff(vals) <= 0.0) if which == "max" else np.all(np.diff(vals) >= 0.0)
    defect = float(np.max(np.abs(vecs.conj() @ vecs.T - np.eye(k))))
    print(f"max|theta - w| = {np.max(np.abs(vals - ref[:k])):.3e}  max r = {info['residual']:.3e}  |Y^H Y - I|max = {defect:.3e}  "
          f"matvecs = {info['matvecs']}  restarts = {info['restarts']}  status = {info['status']}")
    assert np.max(np.abs(vals - ref[:k])) <= 1e-9
    assert info["residual"] == np.max(info["residuals"])
    assert defect <= tol
    for i in range(k):
        y, th = vecs[i], vals[i]
        host_r = float(np.linalg.norm(p["dense"] @ y - th * y))
        assert info["residuals"][i] <= bound(th, tol) and host_r <= bound(th, tol), (i, info["residuals"][i], host_r)
        level = np.abs(w - w[np.argmin(np.abs(w - th))]) <= 1e-8
        delta = np.min(np.abs(w[~level] - th))
        out_of_level = float(np.linalg.norm(y - U[:, level] @ (U[:, level].conj().T @ y)))
        assert out_of_level <= host_r / delta, (i, out_of_level, host_r, delta)


# ---- 1. known answers with multiplicity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,which", [("CH2_8q", 6, "min"), ("H2O_8q", 8, "min"), ("BEH2_6q", 8, "min"),
                                          ("heisenberg_5q", 4, "min"), ("H2O_8q", 8, "max")])
def test_known_answers_with_multiplicity(problems, case, k, which):
    """CH2_8q k = 6 cuts its two-fold level at index 5 / 6.  Measured |Y^H Y - I|max: see DESIGN 4.14."""
    p = problems[case]
    eng = _engine(p["n"], p["xs"], p["zs"], p["cs"])
    vals, vecs, info = eng.lanczos_multi(k, which)
    _check(p, which, k, vals, vecs, info)
    assert eng.last_kernel_ms() > 0.0


# ---- 2. smallest sizes ---------------------------------------------------------------------------------------------------------
def _small(n):
    import tensorrl_qas_amd as tq
    if n == 1:       # H = Z + 0.5 X
        return np.array([0, 1], np.uint64), np.array([1, 0], np.uint64), np.array([1.0, 0.5]), ["Z", "X"]
    ps, ws = vo.heisenberg_paulis(n)
    xs, zs = tq.hamiltonian.masks_from_strings(ps, n)
    return xs, zs, ws, ps


@pytest.mark.parametrize("n,max_basis", [(1, 128), (2, 128), (3, 128), (2, 2)])
def test_smallest_sizes_full_spectrum(n, max_basis):
    """k = 2^n.  Where the basis holds the whole space every stage ends in a breakdown or in a one-dimensional complement,
    its pair is exact in its space, and the bound is the one test_lanczos_gpu.py holds its smallest sizes to: 1e-12 |H|,
    over every pair.  n = 2 with max_basis = 2 restarts (explicitly: no room for a thick restart) inside the 3-fold
    level of the two-site chain and converges to tol like any larger problem: there the bounds are the project's, 1e-9
    and R = 10 tol max(1, |theta|)."""
    xs, zs, cs, ps = _small(n)
    dense = vo.pauli_dense(ps, cs, n)
    w = np.linalg.eigvalsh(dense)
    norm = max(abs(w[0]), abs(w[-1]))
    k = 1 << n
    eng = _engine(n, xs, zs, cs)
    for which, ref in (("min", w), ("max", w[::-1])):
        vals, vecs, info = eng.lanczos_multi(k, which, max_basis=max_basis)
        host_r = max(float(np.linalg.norm(dense @ vecs[i] - vals[i] * vecs[i])) for i in range(k))
        defect = float(np.max(np.abs(vecs.conj() @ vecs.T - np.eye(k))))
        print(f"n = {n} {which}: max|theta - w| = {np.max(np.abs(vals - ref)):.3e}  host r = {host_r:.3e}  defect = {defect:.3e}  info = {info}")
        assert info["pairs"] == k and info["status"] in (0, 1)
        if max_basis >= k:
            assert info["restarts"] == 0 and info["matvecs"] <= k * (k + 1) // 2
            assert np.max(np.abs(vals - ref)) <= 1e-12 * norm
            assert info["residual"] <= 1e-12 * norm and host_r <= 1e-12 * norm
        else:
            assert info["restarts"] >= 1
            assert np.max(np.abs(vals - ref)) <= 1e-9
            for i in range(k):
                assert info["residuals"][i] <= bound(vals[i]) and np.linalg.norm(dense @ vecs[i] - vals[i] * vecs[i]) <= bound(vals[i])
        assert defect <= TOL


# ---- 3. restarts in a tiny basis -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_basis", [4, 8])
@pytest.mark.parametrize("case", ["BEH2_6q", "CH2_8q"])
def test_restarts_in_a_tiny_basis(problems, case, max_basis):
    """k = 3 through thick restarts; and for k = 1 fewer H applications than the explicit restart of vqe_lanczos at the
    same max_basis, tol and seed (same start vector).  Measured: see DESIGN 4.14."""
    p = problems[case]
    eng = _engine(p["n"], p["xs"], p["zs"], p["cs"])
    vals, vecs, info = eng.lanczos_multi(3, "min", max_basis=max_basis, max_matvec=20000)
    _check(p, "min", 3, vals, vecs, info)
    assert info["restarts"] >= 1
    one, vec1, info1 = eng.lanczos_multi(1, "min", max_basis=max_basis, max_matvec=20000)
    _check(p, "min", 1, one, vec1, info1)
    old, _, info0 = eng.lanczos("min", want_vector=False, max_basis=max_basis, max_matvec=20000)
    print(f"{case} max_basis {max_basis}: k = 1 thick restart {info1['matvecs']} applications ({info1['restarts']} restarts), "
          f"vqe_lanczos {info0['matvecs']} ({info0['restarts']} restarts)")
    assert info0["status"] == 0 and abs(old - one[0]) <= 1e-9
    assert info1["restarts"] >= 1 and info1["matvecs"] < info0["matvecs"]


# ---- 4. streaming sizes ----------------------------------------------------------------------------------------------------------
def test_streaming_sizes():
    """heisenberg(14), k = 3, against scipy eigsh on a LinearOperator of hamiltonian.apply (complex arithmetic, its own
    implicitly restarted Lanczos - independent of the kernels)."""
    import tensorrl_qas_amd as tq
    from scipy.sparse.linalg import LinearOperator, eigsh
    n = 14
    ham, _ = tq.hamiltonian.heisenberg(n)
    op = LinearOperator((1 << n, 1 << n), matvec=lambda v: tq.hamiltonian.apply(ham, np.asarray(v, np.complex128).reshape(-1)),
                        dtype=np.complex128)
    ref = np.sort(eigsh(op, k=3, which="SA", return_eigenvectors=False, tol=1e-12))
    eng = _engine(n, ham.xmask, ham.zmask, ham.coeff)
    vals, vecs, info = eng.lanczos_multi(3, "min")
    print(f"n = {n}: theta - eigsh = {vals - ref}  info = {info}  {eng.last_kernel_ms():.2f} ms")
    assert info["pairs"] == 3 and info["status"] == 0
    assert np.max(np.abs(vals - ref)) <= 1e-9
    for i in range(3):
        host_r = float(np.linalg.norm(tq.hamiltonian.apply(ham, vecs[i]) - vals[i] * vecs[i]))
        assert info["residuals"][i] <= bound(vals[i]) and host_r <= bound(vals[i])
    assert np.max(np.abs(vecs.conj() @ vecs.T - np.eye(3))) <= TOL


# ---- 5. bits ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.float64), b[1].view(np.float64))
            and {k: v for k, v in a[2].items() if k != "residuals"} == {k: v for k, v in b[2].items() if k != "residuals"}
            and np.array_equal(a[2]["residuals"], b[2]["residuals"]))


def test_two_calls_return_equal_bits_and_dev_agrees(problems):
    import torch
    p = problems["BEH2_6q"]
    eng = _engine(p["n"], p["xs"], p["zs"], p["cs"])
    a = eng.lanczos_multi(4, "min", max_basis=8)          # restarts included
    b = eng.lanczos_multi(4, "min", max_basis=8)
    assert a[2]["restarts"] >= 1 and _same(a, b)
    buf = torch.empty((4, 1 << p["n"]), dtype=torch.complex128, device="cuda:0")      # no fill kernel on another stream
    vals, info = eng.lanczos_multi_dev(buf.data_ptr(), 4, "min", max_basis=8)
    eng.sync()
    assert _same(a, (vals, buf.cpu().numpy(), info))
    c = eng.lanczos_multi(4, "min", max_basis=8, seed=77)
    assert np.max(np.abs(c[0] - a[0])) <= 1e-9 and not np.array_equal(c[1].view(np.float64), a[1].view(np.float64))
    # the old entry point after the new one on the same handle: its bits are those of a fresh handle
    fresh = _engine(p["n"], p["xs"], p["zs"], p["cs"]).lanczos("min", max_basis=8)
    again = eng.lanczos("min", max_basis=8)
    assert fresh[0] == again[0] and fresh[2] == again[2] and np.array_equal(fresh[1].view(np.float64), again[1].view(np.float64))


# ---- 6. budget -------------------------------------------------------------------------------------------------------------------
def test_budget_inside_stage_two(problems):
    """The stages of a run do not depend on k, so the run for k = 2 tells where stage 2 begins."""
    p = problems["H2O_8q"]
    eng = _engine(p["n"], p["xs"], p["zs"], p["cs"])
    two = eng.lanczos_multi(2, "min", max_basis=8)
    three = eng.lanczos_multi(3, "min", max_basis=8)
    assert two[2]["matvecs"] + 1 < three[2]["matvecs"]
    vals, vecs, info = eng.lanczos_multi(3, "min", max_basis=8, max_matvec=two[2]["matvecs"] + 1)       # VQE_OK: no exception
    print(f"budget {two[2]['matvecs'] + 1}: info = {info}")
    assert info["status"] == 2 and info["status_name"] == "budget" and info["pairs"] == 2 and info["matvecs"] == two[2]["matvecs"] + 1
    assert vals.shape == (2,) and vecs.shape == (2, 1 << p["n"])
    assert np.array_equal(vals, two[0]) and np.array_equal(vecs.view(np.float64), two[1].view(np.float64))
    for i in range(2):
        host_r = float(np.linalg.norm(p["dense"] @ vecs[i] - vals[i] * vecs[i]))
        assert abs(info["residuals"][i] - host_r) <= 1e-10 and host_r <= bound(vals[i])
    none = eng.lanczos_multi(3, "min", max_basis=8, max_matvec=3)
    assert none[2]["status"] == 2 and none[2]["pairs"] == 0 and none[0].shape == (0,) and none[1].shape == (0, 1 << p["n"])


# ---- 7. handle untouched ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True])
def test_the_call_leaves_the_handle_alone(problems, noisy):
    """The recipe of test_lanczos_gpu.py::test_the_call_leaves_the_handle_alone with the new call in place of the old one."""
    import tensorrl_qas_amd as tq
    p = problems["BEH2_6q"]
    rng = np.random.default_rng(9109)
    circs, thetas = [], []
    for _ in range(3):
        kind, q0, q1, pidx, th = random_gates(p["n"], 10, rng)
        circs.append(tq.Circuit(*with_noise_gates(kind, q0, q1, pidx), th.size))
        thetas.append(th)
    psi0 = rng.normal(size=1 << p["n"]) + 1j * rng.normal(size=1 << p["n"])
    psi0 /= np.linalg.norm(psi0)

    def run(with_solver):
        eng = _engine(p["n"], p["xs"], p["zs"], p["cs"])
        eng.set_init_state(psi0)
        if noisy:
            eng.set_noise(0.3, 0.4, 1234)
        out = []
        eng.batch_load(list(circs), list(thetas))
        eng.batch_run_energy()
        out.append(eng.batch_fetch()[1])
        if with_solver:
            before = eng.debug_counters()
            vals, _, info = eng.lanczos_multi(3, "min", max_basis=8)
            assert np.max(np.abs(vals - p["eigvals"][:3])) <= 1e-9 and info["status"] == 0 and info["restarts"] >= 1
            assert np.array_equal(before, eng.debug_counters())
        out.append(eng.batch_fetch()[1])
        eng.batch_run_energy()
        out.append(eng.batch_fetch()[1])
        eng.set_circuit(circs[0])
        out.append(eng.get_state(thetas[0]).view(np.float64))
        out.append(np.array([eng.energy(thetas[0])]))
        return out

    plain, mixed = run(False), run(True)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)
    if noisy:
        assert not np.array_equal(plain[0], plain[2])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def _raw(eng, **fields):
    from tensorrl_qas_amd import _lib
    o = _lib.LanczosMultiOpts()
    assert eng._lib.vqe_lanczos_multi_default_opts(C.byref(o)) == 0
    for k, v in fields.items():
        setattr(o, k, v)
    k = max(int(o.n_eig), 1)
    ev, res, info = (C.c_double * k)(), (C.c_double * k)(), (C.c_double * 5)()
    rc = eng._lib.vqe_lanczos_multi(eng._h, C.byref(o), ev, None, res, info)
    return rc, (eng._lib.vqe_last_error(eng._h) or b"").decode(), list(ev)


def test_refusals(problems):
    import tensorrl_qas_amd as tq
    p = problems["heisenberg_5q"]
    eng = tq.VQEEngine(p["n"], 0)
    rc, msg, _ = _raw(eng)
    assert rc == ESTATE and "Hamiltonian" in msg
    eng.set_hamiltonian(p["xs"], p["zs"], p["cs"])
    eng.set_term_shard(1, 2)
    rc, msg, _ = _raw(eng)
    assert rc == ESTATE and "shard" in msg
    eng.set_term_shard(0, 1)
    bad = [dict(which=2), dict(which=-1), dict(max_basis=1), dict(max_matvec=0), dict(check_every=0), dict(tol=0.0),
           dict(tol=-1e-10), dict(tol=float("nan")), dict(tol=float("inf")),
           dict(n_eig=0), dict(n_eig=-1), dict(n_eig=33), dict(n_eig=65),        # 2^5 = 32 decides here, 64 below
           dict(keep=-1), dict(keep=127), dict(keep=128), dict(max_basis=8, keep=7), dict(max_basis=2, keep=1)]
    for fields in bad:
        rc, msg, _ = _raw(eng, **fields)
        assert rc == EINVAL and "vqe_lanczos_multi" in msg, (fields, rc, msg)
    rc, _, vals = _raw(eng, n_eig=3, max_basis=8, keep=6)          # the same handle, a correct call at the edge of keep
    assert rc == 0 and np.max(np.abs(np.array(vals) - p["eigvals"][:3])) <= 1e-9
    rc, _, vals = _raw(eng, n_eig=32)                              # ... and at the edge of n_eig
    assert rc == 0 and np.max(np.abs(np.array(vals) - p["eigvals"])) <= 1e-9
    h8 = problems["H2O_8q"]
    e8 = _engine(h8["n"], h8["xs"], h8["zs"], h8["cs"])
    rc, msg, _ = _raw(e8, n_eig=65)
    assert rc == EINVAL and "n_eig" in msg
    # an amplitude shard exists on the streaming path only
    ham, _ = tq.hamiltonian.heisenberg(14)
    e14 = _engine(14, ham.xmask, ham.zmask, ham.coeff)
    e14.set_amplitude_shard(1, 2)
    rc, msg, _ = _raw(e14)
    assert rc == ESTATE and "amplitude" in msg
    e14.set_amplitude_shard(0, 1)
    rc, _, vals = _raw(e14, max_matvec=20)
    assert rc == 0
    with pytest.raises(tq.VQEError):
        eng.lanczos_multi(2, "min", tol=0.0)
    with pytest.raises(tq.VQEError):
        eng.lanczos_multi(0, "min")
    with pytest.raises(TypeError):
        eng.lanczos_multi(2, "min", basis=4)
    with pytest.raises(TypeError):
        eng.lanczos_multi(2, "min", start_from_init=1)


# ---- 9. Python namesakes -----------------------------------------------------------------------------------------------------------
def test_python_namesakes(problems):
    import torch
    import tensorrl_qas_amd as tq
    p = problems["CH2_8q"]
    ham = tq.hamiltonian.PauliHamiltonian(p["n"], p["xs"], p["zs"], p["cs"])
    vals, vecs, info = tq.hamiltonian.lowest_eigenpairs_device(ham, 6)
    _check(p, "min", 6, vals, vecs, info)
    levels = tq.hamiltonian.level_structure(vals, 1e-8)
    print(f"CH2_8q levels: {levels}")
    assert levels[0][1] == 3 and abs(levels[0][0] - (-37.0863)) <= 1e-4
    assert [m for _, m in levels] == [m for _, m in tq.hamiltonian.level_structure(p["eigvals"][:6], 1e-8)]
    tv, tt, ti = tq.hamiltonian.lowest_eigenpairs_device(ham, 6, return_tensor=True)
    assert tt.is_cuda and tt.dtype == torch.complex128 and tuple(tt.shape) == (6, 1 << p["n"])
    assert np.array_equal(tv, vals) and np.array_equal(tt.cpu().numpy().view(np.float64), vecs.view(np.float64))
