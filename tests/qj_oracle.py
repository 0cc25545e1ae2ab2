"""Oracle of the quantum-jump trajectories of a Kraus channel (vqe_set_kraus_traj, csrc/vqe_qjump.h); a helper of
tests/test_kraus_traj_cpu.py and tests/test_kraus_traj_gpu.py, not a test.  numpy only.

A plain state-vector simulation in the physical frame (little-endian: qubit q is bit q of an index), all trajectories
of one evaluation side by side as rows of a (T, 2^n) array; no GF(2) frame, no compiled op list, nothing shared with the
kernels.  A two-qubit operator is indexed by bit(q0) + 2 bit(q1) of the gate's qubits, as in tests/dm_kraus_oracle.py.

The definition it restates (include/vqe_hip.h, vqe_set_kraus_traj):
  u   = noise_uniform_k(noise_key(seed, b, e), ((t + 1) << 44) | g)      g = position of the noise gate in the gate list
  p_k = tr(K_k^+ K_k rho_red),  k = the smallest k with u < p_0 + ... + p_k (accumulated in k order in double), none: the
        last k with p_k > 0;  psi <- K_k psi / sqrt(p_k)
  E   = the mean over t of <psi_t|H|psi_t>, summed in t order."""
import numpy as np

CNOT, RX, RY, RZ, DEPOL1, DEPOL2, RXX, RYY, RZZ = range(9)
PAULI = [np.eye(2, dtype=np.complex128), np.array([[0, 1], [1, 0]], np.complex128),
         np.array([[0, -1j], [1j, 0]], np.complex128), np.array([[1, 0], [0, -1]], np.complex128)]
M64 = (1 << 64) - 1


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def noise_key(seed, b, e):
    k = mix64((seed + 0x9E3779B97F4A7C15 * (b + 1)) & M64)
    return mix64(k ^ ((e * 0xBF58476D1CE4E5B9) & M64))


def noise_uniform_k(key, g):
    k = mix64(key ^ ((g * 0x94D049BB133111EB) & M64))
    return float(k >> 11) * (1.0 / 9007199254740992.0)


def draw(seed, b, e, t, g):
    return noise_uniform_k(noise_key(seed, b, e), ((t + 1) << 44) | g)


def _members(n, qa, qb=None):
    """index array (groups, d): the d = 2 or 4 indices of every group, ordered by the local index"""
    i = np.arange(1 << n)
    if qb is None:
        base = i[((i >> qa) & 1) == 0]
        return np.stack([base, base | (1 << qa)], axis=1)
    base = i[(((i >> qa) & 1) == 0) & (((i >> qb) & 1) == 0)]
    return np.stack([base | ((l & 1) << qa) | ((l >> 1) << qb) for l in range(4)], axis=1)


def apply_local(psi, mem, m):
    """rows of psi <- m on the groups mem; m is (d, d), or (T, d, d) with one matrix per row"""
    sub = psi[:, mem]                                       # (T, groups, d)
    new = np.einsum("ij,tgj->tgi", m, sub) if m.ndim == 2 else np.einsum("tij,tgj->tgi", m, sub)
    out = psi.copy()
    out[:, mem] = new
    return out


def rot_matrix(kind, theta):
    """exp(+i theta/2 P) on one qubit, exp(+i theta/2 P (x) P) on two"""
    if kind in (RX, RY, RZ):
        return np.cos(theta / 2) * PAULI[0] + 1j * np.sin(theta / 2) * PAULI[kind - RX + 1]
    p = PAULI[kind - RXX + 1]
    return np.cos(theta / 2) * np.eye(4) + 1j * np.sin(theta / 2) * np.kron(p, p)


CX = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], np.complex128)      # index = control + 2 target


def energy_pauli(psi, xmask, zmask, coeff):
    """<psi|H|psi> of every row of psi, H = sum_k c_k P_k, P = X (x bit), Z (z bit), Y (both) per qubit"""
    psi = np.atleast_2d(psi)
    i = np.arange(psi.shape[1], dtype=np.uint64)
    e = np.zeros(psi.shape[0])
    for x, z, c in zip(xmask, zmask, coeff):
        x, z = np.uint64(int(x)), np.uint64(int(z))
        par = i & z
        for s in (32, 16, 8, 4, 2, 1):
            par = par ^ (par >> np.uint64(s))
        sign = 1.0 - 2.0 * (par & np.uint64(1)).astype(np.float64)
        ph = 1j ** (bin(int(x & z)).count("1"))
        # P|j> = i^{#Y} (-1)^{parity(j & z)} |j ^ x>
        e += c * np.real(ph * np.einsum("tj,tj->t", psi[:, (i ^ x).astype(np.int64)].conj(), sign * psi))
    return e


def run(psi0, kinds, q0, q1, pidx, theta, K1, K2, ham, seed, b, e, T, ts=None):
    """T trajectories of (stream b, evaluation e).  K1 / K2: Kraus set (k, 2, 2) / (k, 4, 4) of the one- / two-qubit
    slot, None: the slot is the identity.  Returns a dict: states (T, 2^n), energies (T,), mean (summed in t order),
    ks (T, slots): the chosen index at every executed noise gate, slot_kind (slots,): 1 or 2, margin: the smallest
    distance of any u to a boundary of the cumulative distribution, jumps: selections k != 0.
    ``ts``: the trajectory indices to simulate (each in 0 .. T-1; default all of them): the rows of every returned array
    are those trajectories in the order of ``ts``, and mean, margin and jumps are over them alone.  The draw of a
    trajectory does not depend on T."""
    psi0 = np.asarray(psi0, np.complex128)
    n = int(round(np.log2(psi0.size)))
    if ts is not None:
        ts = [int(t) for t in ts]
        assert all(0 <= t < T for t in ts), (ts, T)
        return _run(psi0, n, kinds, q0, q1, pidx, theta, K1, K2, ham, seed, b, e, ts)
    return _run(psi0, n, kinds, q0, q1, pidx, theta, K1, K2, ham, seed, b, e, range(T))


def _run(psi0, n, kinds, q0, q1, pidx, theta, K1, K2, ham, seed, b, e, ts):
    T = len(ts)
    psi = np.tile(psi0, (T, 1))
    key = noise_key(seed, b, e)
    ks, slot_kind, margin = [], [], np.inf
    for g in range(len(kinds)):
        k, a, bq = int(kinds[g]), int(q0[g]), int(q1[g])
        if k == CNOT:
            psi = apply_local(psi, _members(n, a, bq), CX)
        elif k in (RX, RY, RZ):
            psi = apply_local(psi, _members(n, a), rot_matrix(k, float(theta[pidx[g]])))
        elif k in (RXX, RYY, RZZ):
            psi = apply_local(psi, _members(n, a, bq), rot_matrix(k, float(theta[pidx[g]])))
        elif k in (DEPOL1, DEPOL2):
            K = K1 if k == DEPOL1 else K2
            if K is None:
                continue
            K = np.asarray(K, np.complex128)
            mem = _members(n, a) if k == DEPOL1 else _members(n, a, bq)
            sub = psi[:, mem]
            rho = np.einsum("tgi,tgj->tij", sub, sub.conj())                # rho_red[i, j] = sum psi_i conj(psi_j)
            M = np.einsum("kmi,kmj->kij", K.conj(), K)                      # K^+ K
            p = np.real(np.einsum("kij,tji->tk", M, rho))                   # tr(M_k rho_red)
            u = np.array([noise_uniform_k(key, ((t + 1) << 44) | g) for t in ts])
            cum = np.zeros(T)
            sel = np.full(T, -1)
            for kk in range(K.shape[0]):
                cum = cum + p[:, kk]
                margin = min(margin, float(np.min(np.abs(u - cum))))
                sel = np.where((sel < 0) & (u < cum), kk, sel)
            for t in np.nonzero(sel < 0)[0]:                                 # rounding: the last k with p_k > 0
                sel[t] = np.nonzero(p[t] > 0)[0][-1]
            psi = apply_local(psi, mem, K[sel] / np.sqrt(p[np.arange(T), sel])[:, None, None])
            ks.append(sel)
            slot_kind.append(1 if k == DEPOL1 else 2)
        else:
            raise ValueError(k)
    en = energy_pauli(psi, *ham)
    s = 0.0
    for v in en:
        s += float(v)
    ks = np.array(ks, np.int64).T.reshape(T, len(slot_kind))
    return {"states": psi, "energies": en, "mean": s / T, "ks": ks, "slot_kind": np.array(slot_kind, np.int64),
            "margin": margin, "jumps": int(np.count_nonzero(ks))}
