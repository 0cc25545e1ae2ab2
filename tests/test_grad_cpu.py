"""Host side of the adjoint gradient: the three C entry points are exported and declared, and optimizer_kind sorts
scipy method names the way CircuitEnv.step runs them.  Needs no GPU."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_SYMBOLS = ("vqe_energy_grad_batch", "vqe_batch_run_energy_grad", "vqe_batch_fetch_grad")


def test_library_exports_gradient_entry_points():
    from tensorrl_qas_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in GRAD_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    c = ctypes
    assert _lib.SIGNATURES["vqe_energy_grad_batch"] == (c.c_int, [c.c_void_p, c.c_int, _lib.c_f64p, _lib.c_f64p, _lib.c_f64p])
    assert _lib.SIGNATURES["vqe_batch_run_energy_grad"] == (c.c_int, [c.c_void_p])
    assert _lib.SIGNATURES["vqe_batch_fetch_grad"] == (c.c_int, [c.c_void_p, _lib.c_f64p])
    header = open(os.path.join(ROOT, "include", "vqe_hip.h")).read()
    for name in GRAD_SYMBOLS:
        assert f"int {name}(" in header, name


@pytest.mark.parametrize("name,kind", [
    ("COBYLA", "device_cobyla"),
    ("CG", "host_gradient"), ("BFGS", "host_gradient"), ("L-BFGS-B", "host_gradient"), ("TNC", "host_gradient"),
    ("SLSQP", "host_gradient"), ("Newton-CG", "host_gradient"), ("l-bfgs-b", "host_gradient"),
    ("Nelder-Mead", "host_gradient_free"), ("Powell", "host_gradient_free"),
])
def test_optimizer_kind(name, kind):
    from tensorrl_qas_amd.environments._core import optimizer_kind
    assert optimizer_kind(name) == kind


@pytest.mark.parametrize("name", ["dogleg", "trust-ncg", "trust-krylov", "trust-exact", "trust-constr", "adam", "", "SPSA"])
def test_optimizer_kind_refuses(name):
    from tensorrl_qas_amd.environments._core import optimizer_kind
    with pytest.raises(NotImplementedError):
        optimizer_kind(name)
