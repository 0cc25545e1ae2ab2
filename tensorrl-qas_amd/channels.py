"""Kraus sets for the noise slots of the exact channel mode (``VQEEngine.set_noise_kraus``).  Host only,
numpy only: every function returns a complex128 array ``(k, d, d)`` with ``sum_k K_k^+ K_k = 1``, d = 2 for the slot
behind one-qubit gates and d = 4 for the slot behind two-qubit gates.  A two-qubit operator is indexed by
``bit(q0) + 2 * bit(q1)`` of the noise gate's qubits, so ``tensor(Ka, Kb)`` puts ``Ka`` on q0 and ``Kb`` on q1.

The reference's environment classes declare ``['depolarizing', 'two_depolarizing', 'amplitude_damping']`` and its noisy
circuit builder imports qulacs' BitFlipNoise, DephasingNoise and IndependentXZNoise; the generators below are those.

Pauli channels - all of the above but amplitude damping - need no Kraus override: ``pauli_weights`` / ``pauli_twirl`` turn
a Kraus set into the probability table of ``VQEEngine.set_noise_pauli`` (the mode 0 sampler draws from it directly,
DESIGN 4.19), ``pauli_channel`` turns a table back into its Kraus set."""
from __future__ import annotations

import numpy as np

_I = np.eye(2, dtype=np.complex128)
_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)


def _prob(p, name="p"):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{name} must lie in [0, 1]")
    return p


def identity(d: int = 2):
    """The identity channel on one (d = 2) or two (d = 4) qubits."""
    return np.eye(d, dtype=np.complex128)[None]


def depolarizing(p):
    """rho -> (1 - p) rho + p/3 (X rho X + Y rho Y + Z rho Z): qulacs DepolarizingNoise, the built-in one-qubit slot."""
    p = _prob(p)
    return np.stack([np.sqrt(1.0 - p) * _I] + [np.sqrt(p / 3.0) * P for P in (_X, _Y, _Z)])


def two_qubit_depolarizing(p):
    """rho -> (1 - p) rho + p/15 sum over the 15 non-identity Pauli pairs: qulacs TwoQubitDepolarizingNoise."""
    p = _prob(p)
    paulis = (_I, _X, _Y, _Z)
    K = [np.sqrt(1.0 - p) * np.eye(4, dtype=np.complex128)]
    for b in range(4):
        for a in range(4):
            if a or b:
                K.append(np.sqrt(p / 15.0) * np.kron(paulis[b], paulis[a]))
    return np.stack(K)


def amplitude_damping(gamma):
    """|1> decays to |0> with probability gamma: |1><1| -> diag(gamma, 1 - gamma).  Not unital."""
    g = _prob(gamma, "gamma")
    return np.array([[[1, 0], [0, np.sqrt(1.0 - g)]], [[0, np.sqrt(g)], [0, 0]]], dtype=np.complex128)


def dephasing(p):
    """Z with probability p: qulacs DephasingNoise."""
    p = _prob(p)
    return np.stack([np.sqrt(1.0 - p) * _I, np.sqrt(p) * _Z])


def bit_flip(p):
    """X with probability p: qulacs BitFlipNoise."""
    p = _prob(p)
    return np.stack([np.sqrt(1.0 - p) * _I, np.sqrt(p) * _X])


def independent_xz(p):
    """X and Z independently, each with probability p: qulacs IndependentXZNoise (a bit flip composed with a dephasing)."""
    p = _prob(p)
    return np.stack([(1.0 - p) * _I, np.sqrt(p * (1.0 - p)) * _X, np.sqrt(p * (1.0 - p)) * _Z, p * (_X @ _Z)])


def tensor(Ka, Kb):
    """The product channel on two qubits: ``Ka`` on q0 (the low index bit), ``Kb`` on q1."""
    Ka, Kb = np.asarray(Ka, np.complex128), np.asarray(Kb, np.complex128)
    if Ka.ndim != 3 or Kb.ndim != 3 or Ka.shape[1:] != (2, 2) or Kb.shape[1:] != (2, 2):
        raise ValueError("tensor takes two one-qubit Kraus sets (k, 2, 2)")
    return np.stack([np.kron(b, a) for a in Ka for b in Kb])


def _paulis(d):
    """The d^2 Pauli matrices in code order: index k = a for d = 2, k = a | b << 2 for d = 4 (a on q0, the low index bit)."""
    one = (_I, _X, _Y, _Z)
    if d == 2:
        return np.stack(one)
    if d == 4:
        return np.stack([np.kron(one[b], one[a]) for b in range(4) for a in range(4)])
    raise ValueError("a Pauli channel acts on one (d = 2) or two (d = 4) qubits")


def pauli_channel(w):
    """The Kraus set of a Pauli channel: ``w`` holds the 3 probabilities of X, Y, Z, or the 15 of the two-qubit codes
    ``k = a | b << 2`` (a on q0, b on q1, 1 = X, 2 = Y, 3 = Z).  Returns ``sqrt(w_0) 1`` first, w_0 the remainder, then
    ``sqrt(w_k) P_k`` in code order - the set ``VQEEngine.set_noise_pauli(w)`` runs in mode 1 and on quantum jumps."""
    w = np.asarray(w, np.float64)
    if w.shape not in ((3,), (15,)):
        raise ValueError("pauli_channel takes 3 or 15 probabilities")
    tot = 0.0
    for x in w:                     # (in this order: the total the engine computes)
        tot += float(x)
    if not (np.all((w >= 0.0) & (w <= 1.0)) and tot <= 1.0 + 1e-12):
        raise ValueError("probabilities must lie in [0, 1] and sum to at most 1")
    P = _paulis(2 if w.size == 3 else 4)
    s = np.sqrt(np.concatenate([[max(0.0, 1.0 - tot)], w]))
    return s[:, None, None] * P


def pauli_twirl(K):
    """The Pauli twirl of a channel: the 3 (d = 2) or 15 (d = 4) probabilities ``w_P = sum_k |tr(P K_k)|^2 / d^2`` of the
    non-identity Paulis in code order (``pauli_channel``'s), for ``VQEEngine.set_noise_pauli``.  The identity's
    probability is the remainder.  A Pauli channel is its own twirl."""
    K = np.asarray(K, np.complex128)
    if K.ndim != 3 or K.shape[1] != K.shape[2] or K.shape[1] not in (2, 4):
        raise ValueError("a Kraus set has shape (k, d, d), d = 2 or 4")
    d = K.shape[1]
    t = np.einsum("pij,kji->pk", _paulis(d), K)
    return (np.sum(np.abs(t) ** 2, axis=1) / d ** 2)[1:]


def pauli_weights(K, tol: float = 1e-12):
    """The weights (as ``pauli_twirl`` orders them) of a Kraus set that IS a Pauli channel, else ``None``.  Decided on
    the channel, not on the form of its operators: the Pauli transfer matrix ``R_ij = tr(P_i E(P_j)) / d`` of a Pauli
    channel is diagonal, and a completely positive map with a diagonal R is a Pauli channel."""
    K = np.asarray(K, np.complex128)
    if K.ndim != 3 or K.shape[1] != K.shape[2] or K.shape[1] not in (2, 4):
        raise ValueError("a Kraus set has shape (k, d, d), d = 2 or 4")
    d = K.shape[1]
    P = _paulis(d)
    EP = np.einsum("kab,jbc,kdc->jad", K, P, K.conj())            # E(P_j) = sum_k K_k P_j K_k^+
    R = np.einsum("iab,jba->ij", P, EP) / d
    if np.max(np.abs(R - np.diag(np.diag(R)))) > tol or abs(R[0, 0] - 1.0) > tol:
        return None
    return pauli_twirl(K)


def is_trace_preserving(K, tol: float = 1e-12) -> bool:
    """max |sum_k K_k^+ K_k - 1| <= tol (the test vqe_set_noise_kraus applies)."""
    K = np.asarray(K, np.complex128)
    if K.ndim != 3 or K.shape[1] != K.shape[2]:
        raise ValueError("a Kraus set has shape (k, d, d)")
    s = np.einsum("kmr,kmc->rc", K.conj(), K)
    return bool(np.max(np.abs(s - np.eye(K.shape[1]))) <= tol)
