"""Case tables and helpers of tests/test_scale_gpu.py and tests/test_scale_cases_cpu.py: the kernels at the batch sizes
the product runs them at - every CU filled to its residency and a second round begun - and device buffers whose
largest offset lies beyond 4 GiB.

The pattern: K distinct circuits, tiled to B = grid + 3 circuits in a fixed shuffled order (tile_order), grid = CUs x
workgroups per CU as device_info() reports them after a first launch of the same kind.  Every copy of a circuit must give
the same bits in every output (assert_copies_identical), and each distinct circuit, taken at its LAST position in the
batch, must agree with the oracle at the project's tolerance (assert_close).  The oracle is paid once per distinct
circuit, the device once per copy.

Nothing here touches the GPU at import; inputs come from lds_cases.py / helpers.py with fixed seeds."""
import functools

import numpy as np

import lds_cases as lc
from helpers import random_gates, random_hamiltonian, random_state, with_noise_gates

LINE = 1 << 32                           # the 4 GiB line, in bytes and in elements
LDS_SIZES = (5, 8, 9, 10, 12, 13)        # fewer amplitudes than lanes; one wave + unit path; last plain-LDS size;
                                         # first register size; bench size; 512 threads
WIDE_SIZES = (8, 12)                     # rows context; block context with tiles
NOISE_SEED = 20241020
EXTRA_TRACED = 10                        # traced streams of a noisy minimise run beyond the six pinned positions
MANY_N, MANY_B = 4, 70001                # more workgroups than 65 535


# ---- the batch layout -----------------------------------------------------------------------------------------------
def pinned_positions(grid):
    """Where copies of circuit 0 sit in a batch of grid + 3: the first two workgroups, the last of the first round, the
    first two of the second and the end of the batch."""
    B = grid + 3
    return sorted({p for p in (0, 1, grid - 1, grid, grid + 1, B - 1) if 0 <= p < B})


def tile_order(K, grid, seed=0):
    """-> order[B], B = grid + 3: which of the K circuits sits at each position.  Circuit 0 at pinned_positions(grid);
    everywhere else a seeded draw that differs from both neighbours."""
    assert K >= 3 and grid >= 1
    B = grid + 3
    order = np.full(B, -1, np.int64)
    order[pinned_positions(grid)] = 0
    rng = np.random.default_rng(9000 + seed)
    for i in range(B):
        if order[i] >= 0:
            continue
        ban = {int(order[i - 1])} if i else set()
        if i + 1 < B and order[i + 1] >= 0:
            ban.add(int(order[i + 1]))
        order[i] = int(rng.choice([k for k in range(K) if k not in ban]))
    return order


def last_positions(order, K):
    """-> the last position of each of the K circuits"""
    return [int(np.nonzero(order == k)[0][-1]) for k in range(K)]


def split(flat, sizes):
    """The concatenated per-circuit layout of batch_fetch's x -> one array per circuit"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [flat[off[b]:off[b + 1]] for b in range(len(sizes))]


# ---- the two comparisons --------------------------------------------------------------------------------------------
def _bits(v):
    return np.ascontiguousarray(v).tobytes()


def assert_copies_identical(order, outputs):
    """outputs: {name: one value or array per batch position}.  Every copy of a circuit has the same BITS in every output
    as the first copy (-0.0 differs from 0.0, a NaN equals itself).  -> the number of copy groups compared."""
    order = np.asarray(order)
    groups = 0
    for k in np.unique(order):
        pos = np.nonzero(order == k)[0]
        if pos.size < 2:
            continue
        groups += 1
        for name, vals in outputs.items():
            assert len(vals) == order.size, (name, len(vals), order.size)
            ref = _bits(vals[pos[0]])
            for p in pos[1:]:
                if _bits(vals[p]) != ref:
                    raise AssertionError(f"{name}: circuit {int(k)} at position {int(p)} differs from its copy at "
                                         f"position {int(pos[0])}: {vals[p]!r} != {vals[pos[0]]!r}")
    return groups


def assert_close(label, got, ref, tol):
    """max |got - ref| <= tol (real or complex entries), or an AssertionError that names the figures.  -> the deviation"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    dev = float(np.abs(got - ref).max(initial=0.0))
    if not dev <= tol:
        raise AssertionError(f"{label}: deviation {dev:.3e} from the oracle exceeds {tol:.1e}")
    return dev


def grad_scale(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


# ---- A. circuits of the LDS-resident family -------------------------------------------------------------------------
def small_p(n):
    return min(3 * n, 10)                 # _small_p of tests/test_lds_sizes_gpu.py


def energy_lengths(n):
    """Gate counts of the energy cases: the grad test's and the energy test's lengths of the size tests (the longest
    they use at this n) and shorter ones down to four gates."""
    return (4, 11, 19, min(12 + 3 * n, 40), min(20 + 4 * n, 70))


def grad_lengths(n):
    return (4, 11, 19, 23, min(12 + 3 * n, 40))


@functools.lru_cache(maxsize=None)
def _random_circuits(n, lengths, seed):
    """random_gates of each length; the first seed of a length whose parameter count is at least one and not taken"""
    out, taken = [], set()
    for i, G in enumerate(lengths):
        for j in range(100):
            kind, q0, q1, pidx, th = random_gates(n, G, np.random.default_rng(seed + 1000 * n + i + 100000 * j), p_cnot=0.4)
            if th.size and th.size not in taken:
                break
        taken.add(th.size)
        out.append(((kind, q0, q1, pidx), th))
    return out


def energy_circuits(n):
    """-> [(gates, theta)], K = 5"""
    return _random_circuits(n, energy_lengths(n), 31000)


def grad_circuits(n):
    return _random_circuits(n, grad_lengths(n), 37000)


MIN_P = (3, 5, 8)                          # beside small_p(n) = 10 at every size of LDS_SIZES


def minimize_maxfun(n):
    return small_p(n) + 1 + lc.AFTER_SIMPLEX


def minimize_circuits(n):
    """-> [(gates, theta)], K = 4: first_decided cases of 3, 5, 8 and small_p(n) parameters for the launch's maxfun"""
    mf = minimize_maxfun(n)
    return [lc.cobyla_case(n, P, 41000 + 10 * n + P, maxfun=mf) for P in MIN_P + (small_p(n),)]


def pre_action(gates, P, ng, noisy=False):
    """The circuit the optimiser of an environment step sees when gate ``ng`` is the new one (-1: none): without it,
    and in a noisy circuit without its channel.  -> (gates, indices of the parameters that are variables, the hole or -1)"""
    kind, q0, q1, pidx = gates
    keep = np.ones(kind.size, bool)
    hole = -1
    if ng >= 0:
        keep[ng] = False
        if noisy:
            keep[ng + 1] = False
        if kind[ng] != 0:
            hole = int(pidx[ng])
    sel = [j for j in range(P) if j != hole]
    pp = np.where(pidx[keep] > hole, pidx[keep] - 1, pidx[keep]) if hole >= 0 else pidx[keep]
    return (kind[keep], q0[keep], q1[keep], pp), sel, hole


ENV_KINDS = ("rotation", "none", "cnot", "rotation")      # the new gate of each of the K = 4 circuits
ENV_P = (10, 8, 9, 6)


@functools.lru_cache(maxsize=None)
def env_step_circuits(n):
    """-> [(gates, theta rounded to float32, new gate)], K = 4: a new rotation (theta = 0, a hole with variables on both
    sides), no new gate, a new CNOT, and a shorter circuit with a new rotation; each the first seed whose pre-action
    walk is decided."""
    mf = minimize_maxfun(n)
    out = []
    for b, (what, P) in enumerate(zip(ENV_KINDS, ENV_P)):
        def build(j, b=b, what=what, P=P):
            gates, th = lc.cobyla_circuit(n, P, 43000 + 10 * n + b + 100000 * j)
            th = th.astype(np.float32).astype(np.float64)
            kind = gates[0]
            ng = -1
            if what == "rotation":
                rot = np.nonzero(kind != 0)[0]
                ng = int(rot[rot.size // 2])
                th[gates[3][ng]] = 0.0
            elif what == "cnot":
                cn = np.nonzero(kind == 0)[0]
                ng = int(cn[cn.size // 2]) if cn.size else -1
            pre, sel, _ = pre_action(gates, P, ng)
            return (gates, th, ng), (n, pre, th[sel], mf, None, None)
        out.append(lc.first_decided(build, f"scale env-step n={n} circuit {b}"))
    return out


NOISY_P = (3, 5, 8, 10)
# A traced stream of the noisy minimise run gets a circuit of 8 or 10 parameters: under Pauli errors on most evaluations
# about one seed in two has a decided walk at 10 parameters, one in three at 8, and hardly any at 3 (counted on the CPU).
NOISY_TRACED_P = (8, 10)


def noisy_maxfun(n):
    """The initial simplex and four evaluations beyond it: the host replay of lc.check_trace then follows the whole run
    (every traced stream costs DECIDED_REPS host walks of this length on the CPU, per seed tried)."""
    return small_p(n) + 1 + 4


def noisy_circuit(n, P, stream, maxfun):
    """The first_decided case of P parameters whose noisy walk is decided under the draws of (NOISE_SEED, stream)
    -> (gates WITH channels, theta)"""
    gates, th = _noisy_case(n, P, stream, maxfun)
    return with_noise_gates(*gates), th


@functools.lru_cache(maxsize=None)
def _noisy_case(n, P, stream, maxfun):
    def build(j):
        gates, th = lc.cobyla_circuit(n, P, 47000 + 10 * n + P + 100000 * j)
        return (gates, th), (n, with_noise_gates(*gates), th, maxfun, (NOISE_SEED, stream, lc.P1, lc.P2), None)
    return lc.first_decided(build, f"scale noisy n={n} P={P} stream={stream}")


def noisy_energy_circuits(n):
    """-> [(gates WITH channels, theta)], K = 4 (no walk: any seed will do)"""
    out = []
    for P in NOISY_P:
        gates, th = lc.cobyla_circuit(n, P, 47000 + 10 * n + P)
        out.append((with_noise_gates(*gates), th))
    return out


def traced_positions(grid):
    """The streams of a noisy minimise run whose traces are checked: the pinned positions + EXTRA_TRACED more"""
    B = grid + 3
    pin = pinned_positions(grid)
    rest = [p for p in range(B) if p not in pin]
    rng = np.random.default_rng(515)
    more = sorted(int(p) for p in rng.choice(rest, min(EXTRA_TRACED, len(rest)), replace=False))
    return pin + more


WIDE_P = (65, 40, 65, 40)


def wide_maxfun():
    return 65 + 1 + 8


def wide_circuits(n):
    """-> [(gates, theta)], K = 4: two circuits just above 64 parameters beside two of 40"""
    mf = wide_maxfun()
    return [lc.cobyla_case(n, P, 51000 + 10 * n + i, maxfun=mf) for i, P in enumerate(WIDE_P)]


def wide_class(n, P):
    """(class, pad) of a circuit of P parameters in a WIDE launch: test_device_cobyla_wide's for P > 64; a circuit of 40
    runs the rows context on the global scratch at one-wave sizes (test_small_circuit_in_a_wide_batch) and is staged in
    the dead state region from 10 qubits (its arrays fit 16 << n bytes)."""
    if P > 64:
        return ("rows" if n <= 9 else "block"), (8 if n in (10, 11) else 16)
    return ("rows", 16) if n <= 9 else ("staged", 8)


def many_circuits():
    """n = 4, K = 4"""
    return _random_circuits(MANY_N, (3, 9, 17, 30), 53000)


# ---- B. buffers beyond 4 GiB ----------------------------------------------------------------------------------------
STREAM_N, STREAM_B = 18, 1030
STREAM_LENGTHS = (9, 12, 15)              # K = 3, G about 12
BENCH_N, BENCH_B = 20, 260
BENCH_LENGTHS = (10, 13)                  # K = 2
STREAM_MAXFUN = 6
STREAM_MIN_P = (4, 7, 9)
AMP_BYTES = 16


def stream_order(K, B, seed=0):
    """The layout of a streaming batch of B states: tile_order with B - 3 in the grid's place (K = 2: the pinned
    positions hold circuit 0 and the rest alternates, beginning with circuit 1)."""
    if K >= 3:
        return tile_order(K, B - 3, seed)
    order = np.full(B, -1, np.int64)
    order[pinned_positions(B - 3)] = 0
    for i in range(B):
        if order[i] < 0:
            order[i] = 1 - order[i - 1]
    return order


@functools.lru_cache(maxsize=None)
def stream_state(n):
    """The initial state of lds_cases.inputs(n): the one lc.cobyla_case decides its walks on"""
    return lc.inputs(n)[0]


@functools.lru_cache(maxsize=None)
def stream_hamiltonian(n, which):
    """"heisenberg": the package's open chain (what bench.py's heis20 object evaluates at n = 20); "random": 24 Pauli
    strings with complex weights."""
    if which == "heisenberg":
        import tensorrl_qas_amd as tq
        h, _ = tq.hamiltonian.heisenberg(n)
        return (np.array(h.xmask, np.uint64), np.array(h.zmask, np.uint64), np.array(h.coeff, np.float64))
    return random_hamiltonian(n, 24, np.random.default_rng(62000 + n), real=False)


def stream_circuits(n, lengths):
    out = []
    for i, G in enumerate(lengths):
        kind, q0, q1, pidx, th = random_gates(n, G, np.random.default_rng(63000 + 100 * n + i), p_cnot=0.3)
        out.append(((kind, q0, q1, pidx), th))
    return out


def stream_oracle_energy(n, gates, th, ham):
    import c_oracle as co
    return co.energy_pauli(n, co.run_circuit(n, stream_state(n), *gates, th), *ham)


def stream_shift_grad(n, gates, th, ham):
    from helpers import shift_grad
    energy = lambda p0, k, a, b, p, t, h: stream_oracle_energy(n, (k, a, b, p), t, h)
    return shift_grad(stream_state(n), *gates, np.asarray(th, np.float64), ham, energy)


# ---- the exact channel mode, batched: 18 resident density matrices of 256 MiB ----------------------------------------
DM_N, DM_B = 12, 18
DM_NOISE = (0.01, 0.05)                    # the noisy environments' strengths
DM_MAXFUN = 4
DM_RANDOM_GATES = (5, 8, 11)               # beside the required pairs: three lengths


@functools.lru_cache(maxsize=None)
def dm_problem():
    """As tests/test_dm_large_gpu.py: the three covering partitions of the qubits, a product state over their common
    refinement with its factor states per partition, a Hamiltonian with complex sign-sum coefficients."""
    import dm_factor_oracle as fo
    n = DM_N
    rng = np.random.default_rng(71000 + n)
    three = fo.covering_partitions(n, rng)
    fine = fo.refinement(three)
    psi0, fine_states = fo.product_state(n, fine, rng)
    states = [fo.coarsen(fine, fine_states, parts) for parts in three]
    ham = random_hamiltonian(n, 30, rng, real=False)
    return three, states, psi0, ham


@functools.lru_cache(maxsize=None)
def dm_circuits():
    """K = 3, one circuit per partition (kind, q0, q1, pidx, theta) with its channels: CNOTs in both orders between each of
    the two highest qubits and a partner inside its set (windows whose bits reach 10, 11 and n + 10, n + 11 of the matrix
    index), and 5 / 8 / 11 random gates."""
    import dm_factor_oracle as fo
    n = DM_N
    three = dm_problem()[0]
    for j in range(100):      # the first seed with three different gate and parameter counts
        rng = np.random.default_rng(72000 + n + 1000 * j)
        out = []
        for parts, G in zip(three, DM_RANDOM_GATES):
            pairs = []
            for q in (n - 1, n - 2):
                mates = [m for m in parts[fo.set_of(parts, q)] if m != q]
                m = n - 2 if q == n - 1 and n - 2 in mates else int(rng.choice(mates))      # the two share a window where they can
                pairs += [(q, m), (m, q)]
            out.append(fo.factor_gates(n, parts, G, rng, p_cnot=0.4, required_pairs=pairs))
        if len({c[4].size for c in out}) == 3 and len({len(c[0]) for c in out}) == 3:
            return out
    raise AssertionError("no seed with three different circuits")


def dm_oracle_energy(k, theta):
    import dm_factor_oracle as fo
    three, states, _, ham = dm_problem()
    return fo.energy(DM_N, three[k], states[k], dm_circuits()[k][:4], theta, ham, *DM_NOISE)


# ---- the Lanczos basis: 260 vectors of 16 MiB ------------------------------------------------------------------------
LZ_N, LZ_BASIS = 20, 260


# ---- the trainable regime: per-circuit COBYLA scratch at circuit x words ----------------------------------------------
TRAIN_N, TRAIN_P, TRAIN_CNOTS = 12, 202, 37      # the shape of test_trainable_scale_12_qubits: rotations with 37 CNOTs among them


def trainable_maxfun():
    return TRAIN_P + 1 + 4


@functools.lru_cache(maxsize=None)
def trainable_circuits():
    """K = 2 circuits of 202 rotations (lc.spread_rotations, a CNOT behind about 37 of them), each the first seed whose
    walk over maxfun evaluations is decided -> [(gates, theta)]"""
    n, P, mf = TRAIN_N, TRAIN_P, trainable_maxfun()
    out = []
    for b in range(2):
        def build(j, b=b):
            kind, q0, q1, pidx, th = lc.spread_rotations(n, P, np.random.default_rng(75000 + b + 100000 * j), p_cnot=TRAIN_CNOTS / P)
            gates = (kind, q0, q1, pidx)
            return (gates, th), (n, gates, th, mf, None, None)
        out.append(lc.first_decided(build, f"scale trainable circuit {b}"))
    return out


@functools.lru_cache(maxsize=None)
def trainable_words():
    """Doubles of the optimiser's arrays of one circuit, from the library's placement rule (host only) for the batch
    sizes of the two circuits"""
    import tensorrl_qas_amd as tq
    sizes = [lc.single_circuit_sizes(g, th.size) for g, th in trainable_circuits()]
    max_ops, max_pair, max_par = (max(s[i] for s in sizes) for i in range(3))
    ng = len(set(lc.inputs(TRAIN_N)[1][0].tolist()))
    q = tq.cobyla_placement(TRAIN_N, max_ops, max_pair, max_par, ng, TRAIN_P, True)
    assert (q["class"], q["pad"]) == ("block", 16), q
    return q["words"]


def trainable_batch(words):
    """B = ceil(2^32 / (8 words)) + 3"""
    return -(-LINE // (8 * words)) + 3


def scratch_stride(words):
    """Doubles between the scratch of two neighbouring circuits: vqe_batch_load keeps the padding-16 layout (``words`` of
    a block-context circuit) + 1 and rounds the running offset to 16 doubles"""
    return (words + 1 + 15) & ~15


# ---- the exact channel gradient: levels + 2 density matrices of ONE circuit -------------------------------------------
DMG_R = 2                                  # the circuit and its twin, both resident
DMG_MIN_LEVELS, DMG_MAX_LEVELS = 15, 17    # (17 + 2) x 2 x 256 MiB = 9.5 GiB


def dm_n_blocks(c):
    """the block count of vqe_dm_plan (host only)"""
    import ctypes as C
    from tensorrl_qas_amd import _lib
    nb = C.c_int32()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib.c_i32p)
    th = np.ascontiguousarray(c[4] if c[4].size else np.zeros(1))
    assert _lib.load().vqe_dm_plan(DM_N, len(c[0]), i32(c[0]), i32(c[1]), i32(c[2]), i32(c[3]), th.ctypes.data_as(_lib.c_f64p),
                                   *DM_NOISE, 0, C.byref(nb), None, None) == 0
    return nb.value


@functools.lru_cache(maxsize=None)
def dm_grad_circuit():
    """One circuit of partition 0 (kind, q0, q1, pidx, theta) whose plan has 15 .. 17 block levels: the first (G, seed)"""
    import dm_factor_oracle as fo
    parts = dm_problem()[0][0]
    for G in range(16, 60, 2):
        for j in range(4):
            rng = np.random.default_rng(77000 + G + 1000 * j)
            pairs = [tuple(int(q) for q in rng.permutation(s)[:2]) for s in parts]
            c = fo.factor_gates(DM_N, parts, G, rng, p_cnot=0.4, required_pairs=pairs)
            if DMG_MIN_LEVELS <= dm_n_blocks(c) <= DMG_MAX_LEVELS and c[4].size >= 4:
                return c
    raise AssertionError("no circuit with 15 .. 17 block levels")


def dm_grad_levels():
    return dm_n_blocks(dm_grad_circuit())


def dm_grad_oracle():
    """-> (E, dE/dtheta) by the factorised exact parameter shift"""
    import dm_factor_oracle as fo
    three, states, _, ham = dm_problem()
    c = dm_grad_circuit()
    return fo.shift_grad(DM_N, three[0], states[0], c[:4], c[4], ham, *DM_NOISE)


# ---- the offline fit: batch x 64 MiB per state-sized buffer ----------------------------------------------------------
FIT_N, FIT_B, FIT_STEPS = 22, 66, 2


# ---- quantum-jump trajectories on the streaming path: one chunk of B x T resident states of 256 KiB ---------------------
TRAJ_N, TRAJ_B, TRAJ_T = 14, 17, 964       # 16 388 states (tests/traj_scale_cases.py): the last four begin past the line


def big_buffers(case):
    """-> {buffer: (elements, bytes per element, stride in elements)} of the device buffers of a case of part B that pass
    the line, from the library's own size rules: StreamWork::states and ::lam hold B states of 2^n amplitudes, stream b
    at b << n (csrc/vqe_stream.h, csrc/vqe_stream_grad.h)."""
    if case == "stream_traj":     # StreamWork::states of sq_eval: the work item w = b T + t of a chunk at (w - w0) << n (csrc/vqe_stream_qjump.h)
        return {"states": (TRAJ_B * TRAJ_T << TRAJ_N, AMP_BYTES, 1 << TRAJ_N)}
    if case == "dm_batched":     # dmb_rho: R resident density matrices of 4^n entries, slot s at s << 2 n (csrc/vqe_dm_batch.h)
        return {"rho": (DM_B << (2 * DM_N), AMP_BYTES, 1 << (2 * DM_N))}
    if case == "trainable_scratch":      # d_scratch: circuit b at scratch_begin[b] = b x stride doubles (load_batch, csrc/vqe_api.hip)
        stride = scratch_stride(trainable_words())
        return {"scratch": (trainable_batch(trainable_words()) * stride, 8, stride)}
    if case == "dm_grad":         # dmb_rho: Lambda, then rho_0 .. rho_levels of the R resident circuits: level l of slot s at
        levels = dm_grad_levels()                                   # ((l + 1) R + s) << 2 n (dm_grad_eval, csrc/vqe_api.hip)
        return {"rho stack": (DMG_R * (levels + 2) << (2 * DM_N), AMP_BYTES, 1 << (2 * DM_N))}
    if case in ("fit_stream", "fit_resident"):      # psi and phi: fit b at b << n (csrc/mps2qc_fit.hip, mps2qc_resident.h)
        out = {"psi": (FIT_B << FIT_N, AMP_BYTES, 1 << FIT_N), "phi": (FIT_B << FIT_N, AMP_BYTES, 1 << FIT_N)}
        G, threads = FIT_N - 1, 256
        if case == "fit_resident":    # sfd_env_partial_count: [fit][gate][block of 256 four-vectors][16]
            out["env partials"] = (FIT_B * G * ((1 << FIT_N) // 4 // threads) * 16, AMP_BYTES, G * ((1 << FIT_N) // 4 // threads) * 16)
        else:                         # d_part: [fit][block of 256 amplitudes][16]
            out["env partials"] = (FIT_B * ((1 << FIT_N) // threads) * 16, AMP_BYTES, ((1 << FIT_N) // threads) * 16)
        return out
    if case == "lanczos":         # LzWork::basis: max_basis vectors, vector k at k << n (csrc/vqe_lanczos.h)
        return {"basis": (LZ_BASIS << LZ_N, AMP_BYTES, 1 << LZ_N)}
    n, B = {"stream_energy": (STREAM_N, STREAM_B), "stream_energy_bench": (BENCH_N, BENCH_B),
            "stream_minimize": (STREAM_N, STREAM_B), "stream_grad": (STREAM_N, STREAM_B),
            "stream_lbfgs": (STREAM_N, STREAM_B)}[case]
    out = {"states": (B << n, AMP_BYTES, 1 << n)}
    if case in ("stream_grad", "stream_lbfgs"):
        out["lambda"] = (B << n, AMP_BYTES, 1 << n)
    return out


BIG_CASES = ("stream_energy", "stream_energy_bench", "stream_minimize", "stream_grad", "stream_lbfgs", "trainable_scratch", "dm_batched",
             "dm_grad", "lanczos", "fit_stream", "fit_resident", "stream_traj")
NOT_CROSSING = ("env partials",)          # counted in a case's memory, not meant to pass the line


def largest_offsets(case):
    """-> {buffer: (largest element offset of the last slice's first element, its byte offset, stride in bytes)}"""
    out = {}
    for name, (elems, size, stride) in big_buffers(case).items():
        first_of_last = elems - stride
        out[name] = (first_of_last, first_of_last * size, stride * size)
    return out


def bytes_needed(case):
    return sum(e * s for e, s, _ in big_buffers(case).values())


def require_memory(case):
    """pytest.skip unless the device has the case's buffers + 2 GiB free"""
    import pytest
    import torch
    need = bytes_needed(case)
    assert need <= 10.5 * 2 ** 30, (case, need)
    free, _ = torch.cuda.mem_get_info()
    if free < need + 2 * 2 ** 30:
        pytest.skip(f"{case}: needs {need / 2 ** 30:.2f} GiB + 2 GiB, the device has {free / 2 ** 30:.2f} GiB free")
    return need
