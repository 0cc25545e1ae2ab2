"""Oracle of the Pauli channel tables of the mode 0 sampler (vqe_set_noise_pauli, csrc/noise_pauli.h); a helper of
tests/test_noise_pauli_cpu.py and tests/test_noise_pauli_gpu.py, not a test.  numpy only.

The definition it restates (include/vqe_hip.h, vqe_set_noise_pauli):
  u     = noise_uniform_k(noise_key(seed, b, e), g)      g = position of the noise gate in the EXECUTED gate list
  cum_k = cum_{k-1} + w_k, cum_0 = 0, in k order in double
  code  = 0 where u >= cum_m, else the smallest k with u < cum_k
with the hash of tests/qj_oracle.py; a slot without a table draws 1 + int(u / p * m) where u < p.  The codes go to
vo.run_circuit(..., noise_draws=codes), which applies code & 3 to q0 and code >> 2 to q1."""
import numpy as np

import qj_oracle as qo
import vqe_oracle as vo

DEPOL1, DEPOL2 = 4, 5


def cumulate(w):
    out, c = [], 0.0
    for x in w:
        c += float(x)
        out.append(c)
    return out


def pauli_code(u, cum):
    """the draw rule, as a search: 0 past the last threshold, else the first k (from 1) with u < cum_k"""
    if not cum or u >= cum[-1]:
        return 0
    for k, c in enumerate(cum):
        if u < c:
            return k + 1
    raise AssertionError("unreachable")


def draws(seed, b, e, kinds, w1=None, w2=None, p1=0.0, p2=0.0):
    """codes[g] of every gate of the executed list `kinds` (0 at the gates that are no noise gates) for (stream b,
    evaluation e), and the smallest distance of a draw to a threshold of the table it was compared with."""
    key = qo.noise_key(seed, b, e)
    cum = {DEPOL1: None if w1 is None else cumulate(w1), DEPOL2: None if w2 is None else cumulate(w2)}
    dep = {DEPOL1: (float(p1), 3), DEPOL2: (float(p2), 15)}
    codes, margin = np.zeros(len(kinds), np.int64), np.inf
    for g, k in enumerate(kinds):
        k = int(k)
        if k not in (DEPOL1, DEPOL2):
            continue
        u = qo.noise_uniform_k(key, g)
        if cum[k] is not None:
            codes[g] = pauli_code(u, cum[k])
            margin = min([margin] + [abs(u - c) for c in cum[k]])
        else:
            p, m = dep[k]
            codes[g] = 1 + int(u / p * m) if u < p else 0
    return codes, margin


def energy(psi0, gates, theta, ham, codes):
    kind, q0, q1, pidx = gates
    return vo.energy_pauli(vo.run_circuit(psi0, kind, q0, q1, pidx, theta, codes), *ham)


def state(psi0, gates, theta, codes):
    kind, q0, q1, pidx = gates
    return vo.run_circuit(psi0, kind, q0, q1, pidx, theta, codes)


def kraus(w):
    """the Kraus set of the table's channel, written down here on its own: sqrt(w_0) 1, then sqrt(w_k) P_b (x) P_a at
    k = a | b << 2 (one qubit: sqrt(w_k) P_k)"""
    w = np.asarray(w, np.float64)
    full = np.concatenate([[max(0.0, 1.0 - cumulate(w)[-1])], w])
    if w.size == 3:
        return np.stack([np.sqrt(full[k]) * qo.PAULI[k] for k in range(4)])
    return np.stack([np.sqrt(full[a | b << 2]) * np.kron(qo.PAULI[b], qo.PAULI[a]) for b in range(4) for a in range(4)])


# ---- the case of the statistics test: 6 qubits, a Z-biased table, a Hamiltonian that tells Z errors from X errors ----
N_SAMPLES = 16384


def stat_case():
    n = 6
    rng = np.random.default_rng(77)
    kind, q0, q1, pidx, th = [], [], [], [], []
    for layer in range(2):
        for q in range(n):
            kind += [2, DEPOL1]; q0 += [q, q]; q1 += [-1, -1]; pidx += [len(th), -1]      # RY
            th.append(rng.uniform(0.3, 1.2))
        for q in range(layer & 1, n - 1, 2):
            kind += [0, DEPOL2]; q0 += [q, q]; q1 += [q + 1, q + 1]; pidx += [-1, -1]      # CNOT
    # H = - sum Z_i Z_i+1 - 0.8 sum X_i: a transverse-field Ising chain
    xs = [0] * (n - 1) + [1 << q for q in range(n)]
    zs = [3 << q for q in range(n - 1)] + [0] * n
    cs = [-1.0] * (n - 1) + [-0.8] * n
    psi0 = np.zeros(1 << n, np.complex128)
    psi0[0] = 1.0
    w1 = np.array([0.004, 0.004, 0.112])
    w2 = np.full(15, 0.002)
    w2[[3 - 1, 12 - 1, 15 - 1]] = 0.05
    return {"n": n, "gates": tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)), "theta": np.array(th), "psi0": psi0,
            "ham": (np.array(xs, np.uint64), np.array(zs, np.uint64), np.array(cs)), "w1": w1, "w2": w2, "seed": 4242}


def stat_exact_values(c):
    """tr(rho H) of the table's channel, of the depolarising channel with the same totals, and without noise"""
    import dm_kraus_oracle as dk
    p1, p2 = cumulate(c["w1"])[-1], cumulate(c["w2"])[-1]
    run = lambda K1, K2: dk.circuit_energy(c["psi0"], *c["gates"], c["theta"], K1, K2, c["ham"])
    return run(kraus(c["w1"]), kraus(c["w2"])), run(dk.depol1(p1), dk.depol2(p2)), run(dk.depol1(0.0), dk.depol2(0.0))


def _w2(entries):
    w = np.zeros(15)
    for code, p in entries.items():
        w[code - 1] = p
    return w


# The tables of the GPU tests: name -> (w1, w2).  Code k = a | b << 2: 1 = X, 2 = Y, 3 = Z on q0 (a) and on q1 (b).
TABLES = {
    # 15 distinct entries and a large total (0.6): most gates draw an error
    "distinct": (np.array([0.2, 0.05, 0.3]), 0.6 * (np.arange(15) + 1.5) / np.sum(np.arange(15) + 1.5)),
    "x_only": (np.array([0.4, 0.0, 0.0]), _w2({1: 0.2, 4: 0.15, 5: 0.1})),
    "y_only": (np.array([0.0, 0.4, 0.0]), _w2({2: 0.2, 8: 0.15, 10: 0.1})),
    "z_only": (np.array([0.0, 0.0, 0.4]), _w2({3: 0.2, 12: 0.15, 15: 0.1})),
    # zeros between non-zero entries
    "gaps": (np.array([0.3, 0.0, 0.2]), _w2({2: 0.1, 3: 0.05, 7: 0.15, 11: 0.1, 14: 0.2})),
    # a total of exactly 1 (every partial sum is a dyadic fraction): every gate draws an error
    "total_one": (np.array([0.5, 0.25, 0.25]), np.array([1.0 / 16] * 14 + [1.0 / 8])),
}
