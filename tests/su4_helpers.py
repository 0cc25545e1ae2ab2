"""Reference for the RXX / RYY / RZZ tests: the unmodified oracle knows CNOT and one-qubit rotations only, so a gate
list with the two-qubit Pauli rotations is expanded by three identities (gates in order of application)

    RXX(a, b, t) = CNOT(a->b), RX(a, t), CNOT(a->b)
    RZZ(a, b, t) = CNOT(a->b), RZ(b, t), CNOT(a->b)
    RYY(a, b, t) = RZ(a, pi/2), RZ(b, pi/2), CNOT(a->b), RX(a, t), CNOT(a->b), RZ(a, -pi/2), RZ(b, -pi/2)

and run through vqe_oracle.run_circuit.  The fixed +-pi/2 angles are two extra parameters behind the circuit's own
(``extend``).  tests/test_su4_cpu.py pins the expansion against the definition cos(t/2) psi + i sin(t/2) P_a P_b psi."""
import numpy as np

import vqe_oracle as vo

RXX, RYY, RZZ = 6, 7, 8


def expand(kind, q0, q1, pidx, n_params, with_source=False):
    """-> (kind, q0, q1, pidx) of the oracle circuit; its parameters are extend(theta).  ``with_source``: also the
    index of the gate each oracle gate came from (noise draws are numbered by the engine's gate positions)."""
    hp, hm = n_params, n_params + 1          # +pi/2, -pi/2
    k2, a2, b2, p2, src = [], [], [], [], []

    def add(k, a, b, p):
        k2.append(k), a2.append(a), b2.append(b), p2.append(p), src.append(g)

    for g, (k, a, b, p) in enumerate(zip(kind, q0, q1, pidx)):
        k, a, b, p = int(k), int(a), int(b), int(p)
        if k == RXX:
            add(0, a, b, -1), add(1, a, -1, p), add(0, a, b, -1)
        elif k == RZZ:
            add(0, a, b, -1), add(3, b, -1, p), add(0, a, b, -1)
        elif k == RYY:
            add(3, a, -1, hp), add(3, b, -1, hp), add(0, a, b, -1), add(1, a, -1, p), add(0, a, b, -1)
            add(3, a, -1, hm), add(3, b, -1, hm)
        else:
            add(k, a, b, p)
    out = tuple(np.array(v, np.int32) for v in (k2, a2, b2, p2))
    return out + (np.array(src, np.int64),) if with_source else out


def extend(theta):
    return np.concatenate([np.asarray(theta, np.float64), [np.pi / 2, -np.pi / 2]])


def run_circuit(psi0, kind, q0, q1, pidx, theta, noise_draws=None):
    """``noise_draws``: one entry per gate of the UNEXPANDED list (vqe_oracle.run_circuit's meaning)."""
    k, a, b, p, src = expand(kind, q0, q1, pidx, len(theta), with_source=True)
    dr = None if noise_draws is None else np.asarray(noise_draws)[src]
    return vo.run_circuit(psi0, k, a, b, p, extend(theta), dr)


def energy(psi0, kind, q0, q1, pidx, theta, ham):
    return vo.energy_pauli(run_circuit(psi0, kind, q0, q1, pidx, theta), *ham)


def shift_grad(psi0, kind, q0, q1, pidx, theta, ham):
    """Exact parameter shift, gate by gate (every generator here is a Pauli string): dE/dtheta_j = sum over the gates
    g with parameter j of (E(theta_g + pi/2) - E(theta_g - pi/2)) / 2, each gate given its own copy of the angle."""
    kind, pidx = np.asarray(kind), np.asarray(pidx)
    rot = [g for g in range(kind.size) if pidx[g] >= 0]
    own = np.full(kind.size, -1, np.int32)
    own[rot] = np.arange(len(rot))
    base = np.array([theta[pidx[g]] for g in rot], np.float64)
    grad = np.zeros(len(theta))
    for i, g in enumerate(rot):
        tp, tm = base.copy(), base.copy()
        tp[i] += np.pi / 2
        tm[i] -= np.pi / 2
        grad[pidx[g]] += 0.5 * (energy(psi0, kind, q0, q1, own, tp, ham) - energy(psi0, kind, q0, q1, own, tm, ham))
    return grad


def random_gates_su4(n, G, rng, p_cnot=0.3, p_two=0.4):
    """All nine gate kinds: CNOT with probability p_cnot, R{XX,YY,ZZ} on a uniform ordered pair with p_two, else
    R{X,Y,Z}; theta ~ U(-pi, pi).  -> (kind, q0, q1, pidx, theta)."""
    kind, q0, q1, pidx, th = [], [], [], [], []
    for _ in range(G):
        u = rng.random()
        if u < p_cnot + p_two and n > 1:
            c = int(rng.integers(n))
            t = int((c + 1 + rng.integers(n - 1)) % n)
            q0.append(c), q1.append(t)
            if u < p_cnot:
                kind.append(0), pidx.append(-1)
                continue
            kind.append(RXX + int(rng.integers(3)))
        else:
            kind.append(1 + int(rng.integers(3))), q0.append(int(rng.integers(n))), q1.append(-1)
        pidx.append(len(th)), th.append(float(rng.uniform(-np.pi, np.pi)))
    return (np.array(kind, np.int32), np.array(q0, np.int32), np.array(q1, np.int32),
            np.array(pidx, np.int32), np.array(th, np.float64))
