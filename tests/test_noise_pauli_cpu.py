"""CPU: Pauli channel tables of the mode 0 sampler (vqe_set_noise_pauli) - everything that needs no device.
* the ABI: the two functions in the header and in the library, a NULL handle refused;
* channels.pauli_weights / pauli_twirl / pauli_channel: the closed forms of the qulacs channels, amplitude damping (no
  Pauli channel; its twirl), the round trip to the same superoperator, trace preservation;
* tests/cpp/noise_pauli_check.cpp, built with g++ -fsanitize=address,undefined and run as a program: pauli_code of the
  shared header csrc/noise_pauli.h against the rule as tests/noise_pauli_oracle.py states it, on every threshold and its
  two neighbouring doubles, with zero-width entries, a total of 1 and an empty table;
* the preconditions of the statistics test of tests/test_noise_pauli_gpu.py on the CPU oracles."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import noise_pauli_oracle as npo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "noise_pauli_check.cpp")
LIB = os.path.join(ROOT, "tensorrl-qas_amd", "libvqe_hip.so")


@pytest.fixture(scope="module")
def ch():
    import tensorrl_qas_amd as tq
    return tq.channels


def superop(K):
    """sum_k K_k (x) conj(K_k): the channel as a matrix on vec(rho)"""
    K = np.asarray(K, np.complex128)
    return sum(np.kron(k, k.conj()) for k in K)


def test_abi():
    header = open(os.path.join(ROOT, "include", "vqe_hip.h")).read()
    for name in ("int vqe_set_noise_pauli(vqe_t* h, const double* w1 /* 3, or NULL */, const double* w2 /* 15, or NULL */);",
                 "int vqe_noise_pauli_info(vqe_t* h, int32_t out[2]);"):
        assert name in header, name
    lib = ctypes.CDLL(LIB)
    for name in ("vqe_set_noise_pauli", "vqe_noise_pauli_info"):
        assert hasattr(lib, name), name
    lib.vqe_set_noise_pauli.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.vqe_noise_pauli_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.vqe_set_noise_pauli(None, None, None) == -22 and lib.vqe_noise_pauli_info(None, None) == -22


def test_pauli_weights_closed_forms(ch):
    p, q = 0.3, 0.2
    assert np.allclose(ch.pauli_weights(ch.depolarizing(p)), [p / 3] * 3, atol=1e-15)
    assert np.allclose(ch.pauli_weights(ch.two_qubit_depolarizing(p)), [p / 15] * 15, atol=1e-15)
    assert np.allclose(ch.pauli_weights(ch.bit_flip(p)), [p, 0, 0], atol=1e-15)
    assert np.allclose(ch.pauli_weights(ch.dephasing(p)), [0, 0, p], atol=1e-15)
    assert np.allclose(ch.pauli_weights(ch.independent_xz(p)), [p * (1 - p), p * p, p * (1 - p)], atol=1e-15)
    # bit flip on q0 (a), dephasing on q1 (b): code a | b << 2 -> X.: 1, .Z: 12, XZ: 13
    w = np.zeros(15)
    w[1 - 1], w[12 - 1], w[13 - 1] = p * (1 - q), (1 - p) * q, p * q
    assert np.allclose(ch.pauli_weights(ch.tensor(ch.bit_flip(p), ch.dephasing(q))), w, atol=1e-15)


def test_amplitude_damping_is_no_pauli_channel_and_its_twirl(ch):
    for g in (0.05, 0.3, 0.9):
        K = ch.amplitude_damping(g)
        assert ch.pauli_weights(K) is None
        assert np.allclose(ch.pauli_twirl(K), [g / 4, g / 4, (1 - g / 2 - np.sqrt(1 - g)) / 2], atol=1e-15)
    assert ch.pauli_weights(ch.tensor(ch.amplitude_damping(0.2), ch.dephasing(0.1))) is None
    # the decision is on the channel, not on the form of the operators: a unitary mixing of a Pauli set is a Pauli channel
    K = ch.dephasing(0.3)
    mixed = np.stack([(K[0] + K[1]) / np.sqrt(2), (K[0] - K[1]) / np.sqrt(2)])
    assert np.allclose(ch.pauli_weights(mixed), [0, 0, 0.3], atol=1e-15)


def test_pauli_channel_round_trip_and_trace(ch):
    sets = [ch.depolarizing(0.1), ch.two_qubit_depolarizing(0.4), ch.bit_flip(0.2), ch.dephasing(0.7), ch.independent_xz(0.25),
            ch.tensor(ch.bit_flip(0.3), ch.dephasing(0.2)), ch.tensor(ch.independent_xz(0.1), ch.depolarizing(0.5))]
    for K in sets:
        w = ch.pauli_weights(K)
        assert w is not None and w.shape == (K.shape[1] ** 2 - 1,)
        assert np.max(np.abs(superop(ch.pauli_channel(w)) - superop(K))) <= 1e-14
    for w1, w2 in npo.TABLES.values():
        for w in (w1, w2):
            K = ch.pauli_channel(w)
            assert K.shape == (w.size + 1, 2 if w.size == 3 else 4, 2 if w.size == 3 else 4)
            assert ch.is_trace_preserving(K, 1e-14)
            assert np.allclose(ch.pauli_weights(K), w, atol=1e-15) and np.allclose(ch.pauli_twirl(K), w, atol=1e-15)
    # the two-qubit order: code a | b << 2 is P_b (x) P_a, q0 the low bit of the matrix index
    K = ch.pauli_channel(np.eye(15)[7 - 1])                      # code 7 = Z on q0 (a = 3), X on q1 (b = 1)
    X, Z = np.array([[0, 1], [1, 0]]), np.diag([1.0, -1.0])
    assert np.array_equal(K[7], np.kron(X, Z)) and not K[:7].any() and not K[8:].any()
    for bad in ([0.5, 0.6, 0.0], [-0.1, 0.2, 0.0], [np.nan, 0.0, 0.0], [0.1] * 4):
        with pytest.raises(ValueError):
            ch.pauli_channel(bad)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("noise_pauli") / "noise_pauli_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tensorrl-qas_amd", "csrc"), SRC, "-o", str(exe)],
                   check=True)
    return str(exe)


def test_pauli_code_of_the_shared_header(checker, tmp_path):
    rng = np.random.default_rng(5)
    tables = [w for pair in npo.TABLES.values() for w in pair]
    tables += [np.array([]), np.zeros(3), np.zeros(15), np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]),
               np.array([0.0, 0.0, 1e-300]), np.array([0.1, 0.2, 0.3]) / 3.0, rng.dirichlet(np.ones(16))[:15],
               rng.dirichlet(np.ones(16))[:15] * (rng.random(15) < 0.5)]
    path = tmp_path / "tables.txt"
    path.write_text("".join(" ".join([str(len(w))] + [float(x).hex() for x in w]) + "\n" for w in tables))
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    cums, n_draws, seen = {}, 0, set()
    for ln in r.stdout.splitlines():
        tok = ln.split()
        if tok[0] == "cum":
            t = int(tok[1])
            cums[t] = [float.fromhex(x) for x in tok[2:]]
            assert cums[t] == npo.cumulate(tables[t]), t                      # the same bits
        elif tok[0] == "draw":
            t, u, code = int(tok[1]), float.fromhex(tok[2]), int(tok[3])
            assert code == npo.pauli_code(u, cums[t]), (t, u, code)
            n_draws += 1
            seen.add((t, code))
    assert len(cums) == len(tables) and n_draws >= sum(4 + 3 * len(w) for w in tables)
    # every entry of positive width is selected somewhere on the grid, none of width 0, and the empty table draws nothing
    for t, w in enumerate(tables):
        assert {c for tt, c in seen if tt == t} - {0} == {k + 1 for k in range(len(w)) if w[k] > 0.0}, t


def test_preconditions_of_the_statistics_test():
    """tests/test_noise_pauli_gpu.py compares the mean of 16 384 sampler evaluations with the exact channel.  That says
    something only where the exact value of the table is far (>= 10 standard errors of such a mean) from both the
    noiseless energy and the depolarising channel of the same totals: checked here on the CPU oracles with the standard
    deviation of 512 oracle-drawn evaluations."""
    c = npo.stat_case()
    e_tab, e_dep, e_clean = npo.stat_exact_values(c)
    es = np.array([npo.energy(c["psi0"], c["gates"], c["theta"], c["ham"],
                              npo.draws(c["seed"], b, 0, c["gates"][0], c["w1"], c["w2"])[0]) for b in range(512)])
    sem = es.std(ddof=1) / np.sqrt(npo.N_SAMPLES)
    print(f"exact: table {e_tab:.6f} depolarising {e_dep:.6f} noiseless {e_clean:.6f}; sem of {npo.N_SAMPLES} samples {sem:.2e}")
    assert abs(e_tab - e_dep) >= 10 * sem and abs(e_tab - e_clean) >= 10 * sem
    assert abs(es.mean() - e_tab) <= 4 * es.std(ddof=1) / np.sqrt(es.size)
