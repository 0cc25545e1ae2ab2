"""Case tables and helpers of tests/test_traj_scale_gpu.py and tests/test_traj_scale_cases_cpu.py: the quantum-jump
trajectory paths (csrc/vqe_qjump.h, csrc/vqe_stream_qjump.h) at occupancy, at 16 - 20 qubits and past 4 GiB, in the manner
of tests/scale_cases.py.

A work item of a trajectory run is w = b T + t (circuit b, trajectory t).  The LDS-resident kernel is a persistent grid
of G workgroups: workgroup g runs the items g, g + G, g + 2 G, ... one after the other on one LDS image.  The helpers of
the first part name the items at which that reuse can go wrong; qj_oracle.run(ts=...) then simulates those alone.

Nothing here touches the GPU at import; inputs come from qj_cases.py / helpers.py with fixed seeds."""
import functools

import numpy as np

import qj_cases as qc
import qj_oracle as qo
import scale_cases as sc
from helpers import random_hamiltonian, random_state
from su4_helpers import random_gates_su4

T_MAX = 4096                              # the ABI's limit of vqe_set_kraus_traj
WG_PER_CU_MAX = 16                        # the upper bound of launch_traj (csrc/vqe_qjump.hip)
COMBO = "damping+product"                 # both slots non-Pauli, a one-qubit and a two-qubit jump
P1, P2 = 0.03, 0.07                       # the depolarising strengths under the override, as tests/test_kraus_traj_gpu.py

# ---- 1. the LDS-resident path: several items per workgroup -----------------------------------------------------------
LDS_B = 3
LDS_LENGTHS = (8, 14, 24)                 # gates ahead of the noise gates: a later item finds a longer predecessor's records
LDS_SEED = 20261020
WG0_CAP, CHANGE_CAP, SAMPLE = 24, 16, 48
CPU_CUS, CPU_WG = 256, (1, 2, 8, 16)      # the grids the CPU test asserts the margins for


def lds_B(cus):
    """Circuits of the batch: three, and more (the three in turn) on a device so large that three times the ABI's
    limit of trajectories would not fill its largest grid twice (above 383 CUs)"""
    return max(LDS_B, -(-(2 * WG_PER_CU_MAX * cus + 3) // T_MAX))


def lds_T(cus):
    """Trajectories per circuit such that every workgroup of the largest grid the launcher makes runs two items and
    three are left over"""
    return -(-(2 * WG_PER_CU_MAX * cus + 3) // lds_B(cus))


def lds_batch(n, cus):
    """-> psi0, ham, the lds_B(cus) circuits"""
    psi0, ham, three = lds_case(n)
    return psi0, ham, [three[b % LDS_B] for b in range(lds_B(cus))]


@functools.lru_cache(maxsize=None)
def lds_case(n):
    """-> psi0, ham, B = 3 circuits (kind, q0, q1, pidx, theta) of qc.noisy_su4 with 8, 14 and 24 gates"""
    rng = np.random.default_rng(9900 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 14, rng, real=False)
    return psi0, ham, [qc.noisy_su4(n, G, rng) for G in LDS_LENGTHS]


def pinned_items(B, T, G):
    """The first two items, the last of the first round, the first two of the second, the last of the second, the first
    of the third and the end"""
    total = B * T
    return sorted({w for w in (0, 1, G - 1, G, G + 1, 2 * G - 1, 2 * G, total - 1) if 0 <= w < total})


def workgroup_items(g, B, T, G, cap=None):
    """The items workgroup g of a grid of G runs, in its order"""
    seq = list(range(g, B * T, G))
    return seq if cap is None else seq[:cap]


def circuit_change_items(B, T, G, cap=None):
    """In every residue class mod G the first item w >= G whose circuit is not that of w - G: the first of a new circuit
    in a workgroup's sequence (the item that compiles over its predecessor's records).  ``cap``: that many of them,
    evenly spread over the classes."""
    out = []
    for g in range(min(G, B * T)):
        for w in range(g + G, B * T, G):
            if w // T != (w - G) // T:
                out.append(w)
                break
    out.sort()
    if cap is not None and len(out) > cap:
        out = [out[(i * len(out)) // cap] for i in range(cap)]
    return out


def sampled_items(n, B, T, G, count=SAMPLE):
    """A seeded sample of the items of the second and later rounds"""
    rest = np.arange(G, B * T)
    rng = np.random.default_rng(LDS_SEED + 1000 * n + G)
    return sorted(int(w) for w in rng.choice(rest, min(count, rest.size), replace=False))


def selected_items(n, B, T, G):
    """The items of an LDS-path run that are held to the oracle: at most 8 + 24 + 16 + 48"""
    return sorted(set(pinned_items(B, T, G)) | set(workgroup_items(0, B, T, G, WG0_CAP))
                  | set(circuit_change_items(B, T, G, CHANGE_CAP)) | set(sampled_items(n, B, T, G)))


def oracle_items(psi0, ham, circuits, K1, K2, seed, e, T, items):
    """qj_oracle.run on the work items ``items`` (w = b T + t) of evaluation e, one call per circuit
    -> (energies in the order of ``items``, the smallest margin, {w: the state})"""
    items = [int(w) for w in items]
    en = np.empty(len(items))
    margin, states = np.inf, {}
    for b in sorted({w // T for w in items}):
        at = [i for i, w in enumerate(items) if w // T == b]
        c = circuits[b]
        r = qo.run(psi0, c[0], c[1], c[2], c[3], c[4], K1, K2, ham, seed, b, e, T, ts=[items[i] % T for i in at])
        en[at] = r["energies"]
        margin = min(margin, r["margin"])
        for row, i in enumerate(at):
            states[items[i]] = r["states"][row]
    return en, margin, states


def t_ordered_mean(row):
    s = 0.0
    for v in row:
        s += float(v)
    return s / len(row)


# ---- the device COBYLA at occupancy ------------------------------------------------------------------------------------
COBYLA_SIZES = (9, 12)                    # one wave per workgroup; register-resident cosets
COBYLA_T = {9: 4096, 12: 1366}
COBYLA_GATES = 9
# The circuits have 7 or 8 parameters, and no optimiser stops before its initial simplex of P + 1 evaluations and one step
# are through: a run of fewer than 10 evaluations ends both at maxfun.  With rhoend = rhobeg an optimiser stops at the
# first step that would shrink its trust region - at evaluation 10 at the earliest for 8 parameters - and 12 evaluations
# leave the other room to go on.  The seeds are those of a host-side walk (HostCobyla on the oracle's means over all T
# trajectories) in which the two stop at evaluations 10 and 12.
COBYLA_MAXFUN = {9: 12, 12: 12}
COBYLA_RHOEND = 1.0
COBYLA_SEED = {9: 31337, 12: 31337}


def cobyla_circuits(n):
    """The two circuits of test_device_cobyla_and_env_step (tests/test_kraus_traj_gpu.py) at this size"""
    rng = np.random.default_rng(8800 + n)
    return [qc.noisy_su4(n, COBYLA_GATES, rng) for _ in range(2)]


def evaluation_order(nfev):
    """All of 1 .. nfev, in the order in which to ask the oracle which evaluation of a COBYLA run produced its result:
    an oracle mean over T trajectories is the expensive part of the check, and the search stops at the first k that
    fits.  The last evaluation first: a run that stops because its trust region is at rhoend returns its last point, one
    that runs out of evaluations its best, which is seldom early.  Only the order rests on this - a wrong guess costs time."""
    return list(range(nfev, 0, -1))


def cobyla_T(n, B, G):
    """The issue's T, and in any case more items than a grid of G workgroups takes in one round"""
    return min(T_MAX, max(COBYLA_T[n], G // B + 1))


# ---- 2. the streaming path at 16, 18 and 20 qubits ---------------------------------------------------------------------
STREAM_SIZES = (16, 18, 20)
STREAM_LENGTHS = (5, 7)
STREAM_T = 2
STREAM_SEED = 20261021


def stream_combos(n):
    return qc.COMBOS if n == 18 else (COMBO,)


def with_channels(k, a, b, p, th):
    """A noise gate behind every gate, as qc.noisy_su4 places them"""
    kind, q0, q1, pidx = [], [], [], []
    for kk, aa, bb, pp in zip(k, a, b, p):
        two = int(kk) in (0, 6, 7, 8)
        kind += [int(kk), 5 if two else 4]
        q0 += [int(aa), int(aa)]
        q1 += [int(bb), int(bb) if two else -1]
        pidx += [int(pp), -1]
    return tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)) + (np.asarray(th, np.float64),)


def gate_classes(kind):
    """Which of a CNOT, a one-qubit rotation and a two-qubit rotation a gate list holds"""
    ks = set(int(v) for v in kind)
    return {"cnot": 0 in ks, "rot1": bool(ks & {1, 2, 3}), "rot2": bool(ks & {6, 7, 8})}


@functools.lru_cache(maxsize=None)
def stream_case(n):
    """-> psi0, ham, B = 2 circuits of 5 and 7 gates + their noise gates, each with a CNOT, a one-qubit and a two-qubit
    rotation"""
    rng = np.random.default_rng(9700 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 14, rng, real=False)
    circuits = []
    for G in STREAM_LENGTHS:
        while True:
            g = random_gates_su4(n, G, rng)
            if all(gate_classes(g[0]).values()):
                break
        circuits.append(with_channels(*g))
    return psi0, ham, circuits


def noise_gates(c):
    return int(np.count_nonzero((c[0] == 4) | (c[0] == 5)))


# ---- 3. one chunk past the 4 GiB line ----------------------------------------------------------------------------------
BIG_N, BIG_B, BIG_T = sc.TRAJ_N, sc.TRAJ_B, sc.TRAJ_T
BIG_GATES = 6
BIG_CHUNK = 1000                          # run B: 17 chunks, the last of 388
BIG_SEED = 20261022
BIG_SAMPLE = 24
GRID_Y = 65535                            # the clamp of a chunk (sq_eval, csrc/vqe_api.hip)


def cut(c, gates):
    """The first ``gates`` gates of a circuit of qc.noisy_su4 with their noise gates (parameters are numbered in gate
    order, so the cut keeps the first of them)"""
    kind, q0, q1, pidx = (v[:2 * gates] for v in c[:4])
    P = int(pidx.max()) + 1
    assert sorted(int(p) for p in pidx if p >= 0) == list(range(P))
    return kind, q0, q1, pidx, c[4][:P]


@functools.lru_cache(maxsize=None)
def big_case():
    """-> psi0, ham, 17 circuits (the three cut circuits in the order of sc.stream_order), that order"""
    psi0, ham, base = qc.parity_case(BIG_N)
    short = [cut(c, BIG_GATES) for c in base]
    order = sc.stream_order(len(short), BIG_B)
    return psi0, ham, [short[k] for k in order], order


def big_items():
    """The streams of the big chunk that are held to the oracle: both sides of the line, the first and last item of
    the last block of each of the three circuits, a seeded sample"""
    total = BIG_B * BIG_T
    line = sc.LINE // (sc.AMP_BYTES << BIG_N)      # the first stream that begins at 2^32 bytes
    items = {0, 1, line - 1, line, total - 1}
    order = big_case()[3]
    for b in sc.last_positions(order, 3):
        items |= {b * BIG_T, b * BIG_T + BIG_T - 1}
    rng = np.random.default_rng(BIG_SEED)
    items |= set(int(w) for w in rng.choice(total, BIG_SAMPLE, replace=False))
    return sorted(items)
