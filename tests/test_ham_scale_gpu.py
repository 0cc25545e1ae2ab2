"""GPU: Hamiltonians whose scale is far from 1.  The unit path drops sign-sum entries below kUnitZeroTol = 2^-44 times its
group's sum |2 c_k| (csrc/vqe_geo.h, csrc/ham_layout.h): a RELATIVE bound, so multiplying every coefficient by 2^k must
change neither the layout nor - every operation on the coefficients being linear and a power of two exact - one bit of
an energy beyond its exponent.  An absolute threshold anywhere on the way would show as another layout or other bits."""
import numpy as np
import pytest

import vqe_oracle as vo
from helpers import fermionic_hamiltonian, random_gates, random_state, with_noise_gates

pytestmark = pytest.mark.gpu
TOL = 1e-10
SHIFTS = (-20, 0, 14)


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _scaled_runs(tq, n, psi0, ham, circuit, ths, oracle, noise=None):
    """energies [shift][theta] and layouts of one handle per shift; each against the oracle at its own scale"""
    xs, zs, cs = ham
    ref = np.array([oracle(t) for t in ths])                    # at 2^0; the oracle is linear in the coefficients too
    out, layouts = {}, {}
    for k in SHIFTS:
        c = np.ldexp(cs, k)
        eng = tq.VQEEngine(n)
        eng.set_init_state(psi0)
        eng.set_hamiltonian(xs, zs, c)
        if noise:
            eng.set_noise(*noise, 11)
            eng.set_noise_mode(1)
        eng.set_circuit(tq.Circuit(*circuit[:4], circuit[4].size))
        out[k] = eng.energy_batch(ths)
        layouts[k] = eng.hamiltonian_layout()
        bound = TOL * max(1.0, float(np.abs(c).sum()))
        err = np.abs(out[k] - np.ldexp(ref, k)).max()
        print(f"n={n} 2^{k}: worst |dE|={err:.2e} of {bound:.2e}, layout {layouts[k]}")
        assert err <= bound, (k, err, bound)
    for k in SHIFTS:
        assert layouts[k] == layouts[0], (k, layouts)
        assert np.array_equal(out[k], np.ldexp(out[0], k)), (k, out[k], np.ldexp(out[0], k))
    return layouts[0]


def test_unit_path_at_ten_qubits(tq):
    n = 10
    rng = np.random.default_rng(4300)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, 12, 20, rng, 3)
    c = random_gates(n, 40, rng)
    ths = np.concatenate([c[4][None, :], c[4][None, :] + rng.normal(size=(3, c[4].size))])
    lay = _scaled_runs(tq, n, psi0, ham, c, ths, lambda t: vo.energy_pauli(vo.run_circuit(psi0, *c[:4], t), *ham))
    assert lay["units"] > 0 and lay["table_groups"] < len(set(ham[0].tolist()))


def test_streaming_path_at_fourteen_qubits(tq):
    n = 14
    rng = np.random.default_rng(4314)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, 12, 20, rng, 3)
    c = random_gates(n, 20, rng)
    ths = np.stack([c[4], c[4] + rng.normal(size=c[4].size)])
    _scaled_runs(tq, n, psi0, ham, c, ths, lambda t: vo.energy_pauli(vo.run_circuit(psi0, *c[:4], t), *ham))


def test_exact_channel_mode_at_six_qubits(tq):
    n, p1, p2 = 6, 0.01, 0.05
    rng = np.random.default_rng(4306)
    psi0 = random_state(n, rng)
    ham = fermionic_hamiltonian(n, 6, 6, rng, 2)
    base = random_gates(n, 20, rng)
    c = with_noise_gates(*base[:4]) + (base[4],)
    ths = np.stack([c[4], c[4] + rng.normal(size=c[4].size)])
    _scaled_runs(tq, n, psi0, ham, c, ths, lambda t: vo.energy_dm(vo.run_circuit_dm(psi0, *c[:4], t, p1, p2), *ham), noise=(p1, p2))
