"""Shared test helpers: fixtures -> oracle / engine inputs."""
import json
import os

import numpy as np

import vqe_oracle as vo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("H2O_8q", "CH2_8q", "BEH2_6q", "heisenberg_5q")
NAME = {0: "cx", 1: "rx", 2: "ry", 3: "rz"}


def known_answers():
    return json.load(open(os.path.join(GOLDEN, "known_answers.json")))


def load_case(case):
    d = np.load(os.path.join(GOLDEN, f"ham_{case}.npz"))
    n = int(d["n"])
    gates = []
    for nm, a, b, ang in zip(d["gate_name"], d["gate_q0"], d["gate_q1"], d["gate_angle"]):
        nm = NAME[int(nm)]
        gates.append((nm, [int(a), int(b)] if nm == "cx" else [int(a)], None if nm == "cx" else float(ang)))
    return {"n": n, "paulis": [str(s) for s in d["paulis"]], "weights": np.asarray(d["weights"], float),
            "eigvals": np.asarray(d["eigvals"], float), "gates": gates}


def oracle_init_state(case_data):
    n = case_data["n"]
    k, a, b, p, th = vo.qasm_to_gatelist(case_data["gates"])
    psi0 = np.zeros(2 ** n, np.complex128)
    psi0[0] = 1
    return vo.run_circuit(psi0, k, a, b, p, th)


def random_gates(n, G, rng, p_cnot=0.5):
    kind, q0, q1, pidx, th = [], [], [], [], []
    for _ in range(G):
        if rng.random() < p_cnot and n > 1:
            c = int(rng.integers(n))
            t = int((c + 1 + rng.integers(n - 1)) % n)
            kind.append(0), q0.append(c), q1.append(t), pidx.append(-1)
        else:
            kind.append(1 + int(rng.integers(3))), q0.append(int(rng.integers(n))), q1.append(-1)
            pidx.append(len(th)), th.append(float(rng.uniform(-np.pi, np.pi)))
    return (np.array(kind, np.int32), np.array(q0, np.int32), np.array(q1, np.int32),
            np.array(pidx, np.int32), np.array(th, np.float64))


def random_state(n, rng):
    v = rng.normal(size=2 ** n) + 1j * rng.normal(size=2 ** n)
    return v / np.linalg.norm(v)


def random_hamiltonian(n, T, rng, real=True):
    """Random Pauli sum; ``real=True`` keeps #Y even (real symmetric matrix)."""
    xs, zs, cs = [], [], []
    while len(xs) < T:
        x, z = int(rng.integers(2 ** n)), int(rng.integers(2 ** n))
        if real and bin(x & z).count("1") % 2:
            continue
        xs.append(x), zs.append(z), cs.append(float(rng.normal()))
    return np.array(xs, np.uint64), np.array(zs, np.uint64), np.array(cs)


def rotations(n, P, rng, p_cnot=0.15):
    """A circuit with exactly P rotations (and, from two qubits on, CNOTs in between)."""
    kind, q0, q1, pidx = [], [], [], []
    for j in range(P):
        kind.append(1 + int(rng.integers(3))), q0.append(int(rng.integers(n))), q1.append(-1), pidx.append(j)
        if rng.random() < p_cnot and n > 1:
            c = int(rng.integers(n))
            kind.append(0), q0.append(c), q1.append(int((c + 1 + rng.integers(n - 1)) % n)), pidx.append(-1)
    return tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)) + (rng.uniform(-np.pi, np.pi, P),)


def tie_free_gates(n, P, rng):
    """P <= 3 n rotations on DISTINCT (qubit, axis) pairs with CNOTs in between (from two qubits on): no two
    parameters act alike, so COBYLA meets no exact ties (two equal simplex values / equally placed vertices are
    decided by the last bit, i.e. by the order of a sum - not by the algorithm)."""
    pairs = [(q, a) for q in range(n) for a in (1, 2, 3)]
    rng.shuffle(pairs)
    kind, q0, q1, pidx = [], [], [], []
    for j, (q, a) in enumerate(pairs[:P]):
        kind.append(a), q0.append(q), q1.append(-1), pidx.append(j)
        if rng.random() < 0.6 and n > 1:
            c = int(rng.integers(n))
            kind.append(0), q0.append(c), q1.append(int((c + 1 + rng.integers(n - 1)) % n)), pidx.append(-1)
    th = rng.uniform(-np.pi, np.pi, P)
    return tuple(np.array(v, np.int32) for v in (kind, q0, q1, pidx)) + (th,)


def with_noise_gates(kind, q0, q1, pidx):
    """construct_ansatz of the noisy seam: DEPOL2 behind every CNOT, DEPOL1 behind every rotation."""
    k2, a2, b2, p2 = [], [], [], []
    for k, a, b, p in zip(kind, q0, q1, pidx):
        k2 += [int(k), 5 if k == 0 else 4]
        a2 += [int(a), int(a)]
        b2 += [int(b), int(b) if k == 0 else -1]
        p2 += [int(p), -1]
    return tuple(np.array(v, np.int32) for v in (k2, a2, b2, p2))


def oracle_energy(psi0, kind, q0, q1, pidx, th, ham):
    return vo.energy_pauli(vo.run_circuit(psi0, kind, q0, q1, pidx, th), *ham)


def shift_grad(psi0, kind, q0, q1, pidx, th, ham, energy=oracle_energy):
    """Exact parameter shift, gate by gate: dE/dtheta_j = sum over the gates g with parameter j of
    (E(theta_g + pi/2) - E(theta_g - pi/2)) / 2, each gate given its own copy of the angle.  ``energy``: the oracle
    that evaluates E (numpy by default; its C restatement where numpy takes seconds per energy)."""
    P = th.size
    grad = np.zeros(P)
    rot = [g for g in range(kind.size) if kind[g] in (1, 2, 3)]
    # one private parameter per rotation gate, so that shared parameters are shifted one gate at a time
    own = np.array([-1] * kind.size, np.int32)
    for i, g in enumerate(rot):
        own[g] = i
    base = np.array([th[pidx[g]] for g in rot])
    for i, g in enumerate(rot):
        tp, tm = base.copy(), base.copy()
        tp[i] += np.pi / 2
        tm[i] -= np.pi / 2
        d = 0.5 * (energy(psi0, kind, q0, q1, own, tp, ham) - energy(psi0, kind, q0, q1, own, tm, ham))
        grad[pidx[g]] += d
    return grad


STEMS = {
    "H2O_8q": "H2O_8q_geom_H_-0.021_-0.002_0.000;_O_0.835_0.452_0.000;_H_1.477_-0.273_0.000_jordan_wigner",
    "CH2_8q": "CH2_8q_geom_C_0.000_0.000_0.000;_H_1.080_0.000_0.000;_H_-0.225_1.056_0.000_jordan_wigner",
    "BEH2_6q": "BEH2_6q_geom_H_0.000_0.000_-1.330;_Be_0.000_0.000_0.000;_H_0.000_0.000_1.330_jordan_wigner",
    "heisenberg_5q": "heisenberg_5q",
}


def make_data_root(root):
    """Lay the golden fixtures out like the reference's dmrg-to-qc/ directory (mol_data/*.npz,
    init_state_circ/*.qasm) so CircuitEnv can be built from an unmodified config."""
    os.makedirs(os.path.join(root, "mol_data"), exist_ok=True)
    os.makedirs(os.path.join(root, "init_state_circ"), exist_ok=True)
    for case, stem in STEMS.items():
        d = load_case(case)
        np.savez(os.path.join(root, "mol_data", stem + ".npz"), paulis=np.array(d["paulis"]),
                 weights=d["weights"], eigvals=d["eigvals"], energy_shift=0)
        lines = ["OPENQASM 2.0;", 'include "qelib1.inc";', f"qreg q[{d['n']}];"]
        for name, qs, ang in d["gates"]:
            if name == "cx":
                lines.append(f"cx q[{qs[0]}],q[{qs[1]}];")
            else:
                lines.append(f"{name}({ang!r}) q[{qs[0]}];")
        with open(os.path.join(root, "init_state_circ", f"init_{stem}_TNbond2.qasm"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return root


def reference_config(name, data_root):
    conf = json.load(open(os.path.join(GOLDEN, "host_logic.json")))["configs"][name]
    conf = json.loads(json.dumps(conf))
    conf["env"]["data_root"] = data_root
    return conf


def fermionic_hamiltonian(n, n_hop, n_quad, rng, dressed=0):
    """Number-conserving Pauli sum of Jordan-Wigner shape on n qubits (the structure of the molecular Hamiltonians
    the reference ships, reference dmrg-to-qc/mol_data): identity + Z + ZZ terms, ``n_hop`` hopping pairs
    {X Z..Z X, Y Z..Z Y} with equal weights, ``n_quad`` double-excitation octets with the signs of
    a+_p a+_q a_r a_s + h.c., and ``dressed`` hopping pairs multiplied by a number operator (1 - Z_k) / 2.
    Returns (xmask, zmask, coeff) with coeff the coefficient of the Pauli STRING (Y = Y)."""
    terms = {}

    def add(x, z, w):
        terms[(x, z)] = terms.get((x, z), 0.0) + w

    wt = lambda: float(rng.normal() * 10.0 ** (-rng.uniform(0, 2)))
    add(0, 0, wt())
    for q in range(n):
        add(0, 1 << q, wt())
    for a in range(n):
        for b in range(a + 1, n):
            if rng.random() < 0.5:
                add(0, (1 << a) | (1 << b), 0.1 * wt())
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    hop = [pairs[i] for i in rng.choice(len(pairs), min(n_hop + dressed, len(pairs)), replace=False)]
    for i, (a, b) in enumerate(hop):
        zs = sum(1 << k for k in range(a + 1, b))
        w = 0.1 * wt()
        x = (1 << a) | (1 << b)
        if i < n_hop:
            add(x, zs, w), add(x, zs | x, w)
        else:                       # (1 - Z_k) / 2 times the hopping pair, k outside [a, b]
            ks = [k for k in range(n) if k < a or k > b]
            if not ks:
                continue
            k = int(rng.choice(ks))
            for zz, sg in ((zs, 0.5), (zs | (1 << k), -0.5)):
                add(x, zz, sg * w), add(x, zz | x, sg * w)
    quads = [(a, b, c, d) for a in range(n) for b in range(a + 1, n) for c in range(b + 1, n) for d in range(c + 1, n)]
    if quads:
        for i in rng.choice(len(quads), min(n_quad, len(quads)), replace=False):
            a, b, c, d = quads[i]
            zs = sum(1 << k for k in range(a + 1, b)) | sum(1 << k for k in range(c + 1, d))
            x = (1 << a) | (1 << b) | (1 << c) | (1 << d)
            w = 0.05 * wt()
            for ys, sg in (((), 1), ((c, d), -1), ((b, d), 1), ((b, c), 1), ((a, d), 1), ((a, c), 1), ((a, b), -1), ((a, b, c, d), 1)):
                add(x, zs | sum(1 << k for k in ys), sg * w)
    keys = sorted(terms)
    return (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint64),
            np.array([terms[k] for k in keys], np.float64))


class OracleShardBackend:
    """Local arithmetic of the CPU tests of the amplitude-sharded states: the oracle stands in for the GPU (only the
    sharding logic - plan, exchanges, signs of the rank bits - is under test; tensorrl_qas_amd.parallel)."""

    def new_shard(self, values):
        return np.ascontiguousarray(values, np.complex128).copy()

    def apply(self, shard, kind, q0, q1, pidx, theta):
        return vo.run_circuit(shard, kind, q0, q1, pidx, theta)

    def energy(self, shard, xs, zs, cs):
        return vo.energy_pauli(shard, xs, zs, cs) if len(xs) else 0.0

    def halves(self, shard, local_pos):
        return shard.reshape(-1, 2, 1 << local_pos)

    def to_host(self, shard):
        return np.asarray(shard)


MPS2QC_OUTPUTS = ("opt_gates", "final_gates", "loss_history", "best_val", "n_iter", "last_envs", "last_overlap")


def mps2qc_raw_fit(stream, n, sites, target, init, steps, only=MPS2QC_OUTPUTS, frozen=False):
    """One fit through the raw C ABI of libmps2qc_hip.so (3e-3, 0.9, 0.999, 1e-8; tol 1e-30 and param_tol 0: every
    step runs).  ``only``: the outputs that get a pointer, every other one is passed as NULL.  Returns the return
    code and the arrays that were asked for."""
    import ctypes as C
    from tensorrl_qas_amd import _lib
    lib = _lib.load_mps2qc()
    sites = np.ascontiguousarray(sites, np.int32)
    target, init = np.ascontiguousarray(target, np.complex128), np.ascontiguousarray(init, np.complex128)
    B, G = init.shape[0], len(sites)
    out = dict(opt_gates=np.zeros_like(init), final_gates=np.zeros_like(init), loss_history=np.zeros((B, steps)),
               best_val=np.zeros(B), n_iter=np.zeros(B, np.int32), last_envs=np.zeros_like(init),
               last_overlap=np.zeros(B, np.complex128))
    ptr = {k: (v.ctypes.data_as(_lib.c_i32p if k == "n_iter" else _lib.c_f64p) if k in only else None) for k, v in out.items()}
    head = (0, n, G, sites.ctypes.data_as(_lib.c_i32p), B, target.ctypes.data_as(_lib.c_f64p), int(target.ndim == 1),
            init.ctypes.data_as(_lib.c_f64p), 3e-3, 0.9, 0.999, 1e-8, int(frozen), steps, 1e-30, 0.0)
    tail = tuple(ptr[k] for k in MPS2QC_OUTPUTS) + (None,)
    rc = lib.mps2qc_fit_brickwork_stream(*head, *tail) if stream else lib.mps2qc_fit_brickwork(*head, 1, *tail)
    return rc, {k: v for k, v in out.items() if k in only}
