"""GPU: the unit path of the energy step with host-built LDS addresses (HamDev::uaddr).  Energies and states of
Hamiltonians held partly as units against the CPU oracle at every size the unit path serves, and the fused env-step
kernel against the standalone energy kernel bit for bit at every trial point of the device optimiser."""
import numpy as np
import pytest

import vqe_oracle as vo
from helpers import CASES, fermionic_hamiltonian, load_case, random_gates, random_state

pytestmark = pytest.mark.gpu

E_TOL = 1e-10
A_TOL = 1e-12


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _engine(tq, n, psi0, ham):
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    return eng


def _check_energies_and_state(tq, n, psi0, ham, rng, G):
    eng = _engine(tq, n, psi0, ham)
    kind, q0, q1, pidx, th = random_gates(n, G, rng)
    eng.set_circuit(tq.Circuit(kind, q0, q1, pidx, th.size))
    ths = np.concatenate([th[None, :], th[None, :] + rng.normal(size=(3, th.size))])
    got = eng.energy_batch(ths)
    ref = np.array([vo.energy_pauli(vo.run_circuit(psi0, kind, q0, q1, pidx, t), *ham) for t in ths])
    assert np.abs(got - ref).max() < E_TOL, np.abs(got - ref).max()
    psi = eng.get_state(th)
    assert np.abs(psi - vo.run_circuit(psi0, kind, q0, q1, pidx, th)).max() < A_TOL
    return eng


@pytest.mark.parametrize("n", [8, 9, 10, 11, 12, 13])
def test_unit_path_energies_by_size(tq, n):
    rng = np.random.default_rng(7300 + n)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, 2 * n, 3 * n, rng, 3)
    eng = _check_energies_and_state(tq, n, psi0, ham, rng, 40)
    lay = eng.hamiltonian_layout()
    assert lay["units"] > 0 and lay["units"] % 12 == 0


def test_unit_path_bench_hamiltonian(tq):
    n = 12
    rng = np.random.default_rng(7312)
    H = tq.hamiltonian.synthetic_lih12()
    psi0 = tq.hamiltonian.brickwork_state(n, 12)
    eng = _check_energies_and_state(tq, n, psi0, (H.xmask, H.zmask, H.coeff), rng, 64)
    assert eng.hamiltonian_layout()["units"] > 0
    # the bank swizzle of the state's LDS copy lowers the modelled conflicts of the unit reads
    sc = eng.unit_bank_score()
    assert 1.0 <= sc["mean"] < sc["plain_mean"] and sc["worst"] >= 1.0, sc


@pytest.mark.parametrize("case", CASES)
def test_unit_path_golden_hamiltonians(tq, case):
    d = load_case(case)
    n = d["n"]
    xs, zs = tq.hamiltonian.masks_from_strings(d["paulis"], n)
    rng = np.random.default_rng(7400 + n)
    _check_energies_and_state(tq, n, random_state(n, rng), (xs, zs, d["weights"]), rng, 30)


@pytest.mark.parametrize("n,seed", [(8, 0), (10, 1), (12, 2), (13, 3), (12, -1)])
def test_fused_trial_energies_equal_standalone_energies(tq, n, seed):
    """Every trial point of the fused minimiser (vqe_batch_set_trace) re-evaluated by the standalone energy kernel of
    the same handle: the two launch the same energy step, so the values agree bit for bit (seed -1: the bench
    Hamiltonian, whose state copy is bank-swizzled)."""
    rng = np.random.default_rng(7500 + seed)
    psi0 = random_state(n, rng)
    if seed < 0:
        H = tq.hamiltonian.synthetic_lih12()
        ham = (H.xmask, H.zmask, H.coeff)
    else:
        ham = fermionic_hamiltonian(n, 2 * n, 2 * n, rng, 2)
    eng = _engine(tq, n, psi0, ham)
    assert eng.hamiltonian_layout()["units"] > 0
    kind, q0, q1, pidx, th = random_gates(n, 24, rng)
    c = tq.Circuit(kind, q0, q1, pidx, th.size)
    eng.batch_set_trace(True)
    eng.batch_load([c], [th])
    eng.batch_run_minimize(1.0, 1e-4, 60)
    _, _, nd = eng.batch_fetch()
    ft, xt = eng.batch_fetch_trace(0, th.size)
    eng.batch_set_trace(False)
    eng.set_circuit(c)
    nd = int(nd[0])
    assert 1 <= nd <= 60
    assert np.array_equal(ft[:nd], eng.energy_batch(xt[:nd]))
