"""Dense oracle of the exact channel mode with Kraus channels in the noise slots and two-qubit rotations (a helper of
tests/test_dm_channels_cpu.py and tests/test_dm_channels_gpu.py, not a test).

rho is a plain 2^n x 2^n matrix rho[ket, bra] (little-endian: qubit q is bit q of an index).  Every gate is a 2^n x 2^n
matrix U applied as U rho U^+, every channel an explicit Kraus sum  sum_k K_k rho K_k^+  of 2^n x 2^n matrices - no
windows, no superoperators, no fused blocks, so nothing is shared with csrc/dm_host.h and csrc/dm_build.h.  A two-qubit
Kraus operator is indexed by bit(q0) + 2 bit(q1) of the noise gate's qubits, as vqe_set_noise_kraus defines it.
Small n only (the tests stay at n <= 8)."""
import numpy as np

CNOT, RX, RY, RZ, DEPOL1, DEPOL2, RXX, RYY, RZZ = range(9)
PAULI = [np.eye(2, dtype=np.complex128), np.array([[0, 1], [1, 0]], np.complex128),
         np.array([[0, -1j], [1j, 0]], np.complex128), np.array([[1, 0], [0, -1]], np.complex128)]
MAX_QUBITS = 8


def depol1(p):
    """Kraus set of rho -> (1 - p) rho + p/3 sum_P P rho P"""
    return np.stack([np.sqrt(1.0 - p) * PAULI[0]] + [np.sqrt(p / 3.0) * PAULI[k] for k in (1, 2, 3)])


def depol2(p):
    """Kraus set of rho -> (1 - p) rho + p/15 sum over the 15 non-identity Pauli pairs"""
    K = [np.sqrt(1.0 - p) * np.eye(4, dtype=np.complex128)]
    K += [np.sqrt(p / 15.0) * np.kron(PAULI[b], PAULI[a]) for b in range(4) for a in range(4) if a or b]
    return np.stack(K)


def embed1(n, q, m):
    """one-qubit matrix m on qubit q as a 2^n x 2^n matrix"""
    return np.kron(np.eye(1 << (n - 1 - q)), np.kron(m, np.eye(1 << q)))


def embed2(n, qa, qb, m):
    """4 x 4 matrix m, index = bit(qa) + 2 bit(qb), as a 2^n x 2^n matrix"""
    dim = 1 << n
    i = np.arange(dim)
    loc = ((i >> qa) & 1) | (((i >> qb) & 1) << 1)
    rest = i & ~((1 << qa) | (1 << qb))
    full = np.zeros((dim, dim), np.complex128)
    for b in range(4):
        j = rest | ((b & 1) << qa) | ((b >> 1) << qb)
        full[i, j] = m[loc, b]
    return full


def rot1(kind, theta):
    """exp(+i theta/2 P), the convention of the engine and of qulacs"""
    return np.cos(theta / 2) * PAULI[0] + 1j * np.sin(theta / 2) * PAULI[kind - RX + 1]


def rot2(n, kind, qa, qb, theta):
    """exp(+i theta/2 P_qa P_qb) as a 2^n x 2^n matrix"""
    p = PAULI[kind - RXX + 1]
    return np.cos(theta / 2) * np.eye(1 << n) + 1j * np.sin(theta / 2) * (embed1(n, qa, p) @ embed1(n, qb, p))


def run(psi0, kinds, q0, q1, pidx, theta, K1, K2):
    """rho after the gate list: K1 (k, 2, 2) at every DEPOL1 gate, K2 (k, 4, 4) at every DEPOL2 gate"""
    psi0 = np.asarray(psi0, np.complex128)
    n = int(round(np.log2(psi0.size)))
    assert n <= MAX_QUBITS
    rho = np.outer(psi0, psi0.conj())
    cx = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], np.complex128)      # index = control + 2 target
    for g in range(len(kinds)):
        k, a, b = int(kinds[g]), int(q0[g]), int(q1[g])
        if k == DEPOL1:
            ops = [embed1(n, a, m) for m in np.asarray(K1, np.complex128)]
        elif k == DEPOL2:
            ops = [embed2(n, a, b, m) for m in np.asarray(K2, np.complex128)]
        elif k == CNOT:
            ops = [embed2(n, a, b, cx)]
        elif k in (RX, RY, RZ):
            ops = [embed1(n, a, rot1(k, float(theta[pidx[g]])))]
        elif k in (RXX, RYY, RZZ):
            ops = [rot2(n, k, a, b, float(theta[pidx[g]]))]
        else:
            raise ValueError(k)
        rho = sum(m @ rho @ m.conj().T for m in ops)
    return rho


def hamiltonian(n, xmask, zmask, coeff):
    """sum_k c_k P_k as a dense matrix, P = product over the qubits of X (x bit), Z (z bit) or Y (both)"""
    h = np.zeros((1 << n, 1 << n), np.complex128)
    for x, z, c in zip(xmask, zmask, coeff):
        x, z = int(x), int(z)
        term = np.eye(1, dtype=np.complex128)
        for q in range(n - 1, -1, -1):      # kron: the first factor is the highest qubit
            term = np.kron(term, PAULI[(0, 3, 1, 2)[2 * ((x >> q) & 1) + ((z >> q) & 1)]])
        h += c * term
    return h


def energy(rho, xmask, zmask, coeff):
    """tr(rho H)"""
    n = int(round(np.log2(rho.shape[0])))
    return float(np.real(np.trace(rho @ hamiltonian(n, xmask, zmask, coeff))))


def circuit_energy(psi0, kinds, q0, q1, pidx, theta, K1, K2, ham):
    return energy(run(psi0, kinds, q0, q1, pidx, theta, K1, K2), *ham)


def shift_grad(psi0, kinds, q0, q1, pidx, theta, K1, K2, ham):
    """dE/dtheta_j = sum over the gates with parameter j of [E(theta_g + pi/2) - E(theta_g - pi/2)] / 2, each gate
    shifted on its own.  Exact here: every rotation is exp(i theta/2 P) with P^2 = 1, a channel is linear and does not
    depend on the angles."""
    theta = np.asarray(theta, np.float64)
    h = hamiltonian(int(round(np.log2(np.asarray(psi0).size))), *ham)
    rot = [g for g in range(len(kinds)) if int(kinds[g]) in (RX, RY, RZ, RXX, RYY, RZZ)]
    own = np.full(len(kinds), -1, np.int64)
    own[rot] = np.arange(len(rot))
    base = np.array([theta[pidx[g]] for g in rot], np.float64)
    grad = np.zeros(theta.size)
    for i, g in enumerate(rot):
        e = []
        for s in (np.pi / 2, -np.pi / 2):
            t = base.copy()
            t[i] += s
            e.append(float(np.real(np.trace(run(psi0, kinds, q0, q1, own, t, K1, K2) @ h))))
        grad[pidx[g]] += 0.5 * (e[0] - e[1])
    return grad
