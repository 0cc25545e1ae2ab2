"""Circuits of the batched exact channel mode's tests (tests/test_dm_plan_cpu.py, tests/test_dm_batch_gpu.py)."""
import numpy as np

from helpers import random_gates


def noisy(base):
    """a depolarising channel behind every gate, as construct_ansatz of the noisy variants places them
    (the construction of tests/test_dm_gpu.py)"""
    kind, q0, q1, pidx = [], [], [], []
    for k, a, b, p in zip(*base[:4]):
        kind += [k, 5 if k == 0 else 4]
        q0 += [a, a]
        q1 += [b, b if k == 0 else -1]
        pidx += [p, -1]
    return tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)) + (base[4],)


def gate_list(gates):
    """(kind, q0, q1, theta) per gate, theta None for a CNOT -> the five arrays of random_gates"""
    kind, q0, q1, pidx, th = [], [], [], [], []
    for k, a, b, t in gates:
        kind.append(k), q0.append(a), q1.append(b)
        if k == 0:
            pidx.append(-1)
        else:
            pidx.append(len(th)), th.append(float(t))
    return (np.array(kind, np.int32), np.array(q0, np.int32), np.array(q1, np.int32), np.array(pidx, np.int32),
            np.array(th, np.float64))


def mixed_batch(n, G, rng):
    """Five circuits of five different lengths on n qubits (G >= 8): G gates + G channels, a shorter one, one with ZERO
    gates, one with rotations and CNOTs but no noise gates (an odd number of gates; the noisy ones are even), one of
    rotations and their channels only (no CNOT)."""
    a = noisy(random_gates(n, G, rng))
    b = noisy(random_gates(n, G // 3, rng))
    empty = tuple(np.zeros(0, np.int32) for _ in range(4)) + (np.zeros(0),)
    clean = random_gates(n, 2 * (G // 4) + 1, rng)
    rots = noisy(random_gates(n, G // 3 + 1, rng, p_cnot=0.0))
    return [a, b, empty, clean, rots]
