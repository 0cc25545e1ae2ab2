"""The case table of the streaming-path planner tests: named (n, gates, Hamiltonian) inputs, each built to reach one
branch of k_t_plan_ops / k_t_plan_energy (csrc/vqe_tile.h).  tests/test_tile_plan_cpu.py certifies with the planner
model (tests/tile_plan_model.py) that every case reaches the branch its name promises and that the table as a whole
reaches every branch; tests/test_stream_planner_gpu.py runs the same table on the device against the oracle.

A gate is (kind, q0, q1) with the kinds of the C ABI; every rotation gets its own parameter, in gate order.  A
Hamiltonian is (xmask, zmask, coeff).  No GPU, no oracle and no random draw at import beyond seeded numpy generators."""
import zlib

import numpy as np

from tile_plan_model import G_CNOT, G_RX, G_RY, G_RZ, G_RXX, G_RYY, G_RZZ

CX, RX, RY, RZ, RXX, RYY, RZZ = G_CNOT, G_RX, G_RY, G_RZ, G_RXX, G_RYY, G_RZZ
KIND_NAME = {RX: "rx", RY: "ry", RYY: "ryy"}
N = 14
A, B, C = 5, 8, 11          # the slot qubits of the flip-code circuits (all >= kTileLow)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def ham_arrays(terms):
    """[(x, z, c)] -> (xmask, zmask, coeff)"""
    return (np.array([t[0] for t in terms], np.uint64), np.array([t[1] for t in terms], np.uint64),
            np.array([t[2] for t in terms], np.float64))


def random_complex_hamiltonian(n, T, name):
    """T random Pauli strings, odd Y counts allowed (imaginary weights c i^{#Y}), normal coefficients."""
    rng = _rng("ham:" + name)
    return ham_arrays([(int(rng.integers(1 << n)), int(rng.integers(1 << n)), float(rng.normal())) for _ in range(T)])


def H12(n=N):
    return random_complex_hamiltonian(n, 12, "H12:%d" % n)


def gate_arrays(gates):
    """-> (kind, q0, q1, pidx, n_params) as the engine's Circuit and the oracle take them."""
    kind = np.array([g[0] for g in gates], np.int32).reshape(-1)
    q0 = np.array([g[1] for g in gates], np.int32).reshape(-1)
    q1 = np.array([g[2] for g in gates], np.int32).reshape(-1)
    pidx = np.full(kind.size, -1, np.int32)
    pidx[kind != CX] = np.arange(int((kind != CX).sum()))
    return kind, q0, q1, pidx, int((kind != CX).sum())


def ladder(n):
    """CNOT(q, q + 1) down the register: behind it the partner mask of qubit q is e_q ^ e_(q+1), the sign mask of
    qubit q is e_0 ^ .. ^ e_q."""
    return [(CX, q, q + 1) for q in range(n - 1)]


def rotations(qubits, name, kinds=(RX, RY, RZ), pair_first=True):
    """One rotation per entry of ``qubits``; kinds drawn from ``kinds`` by a seeded generator, except that with
    ``pair_first`` the first rotation on a qubit is RX or RY (so that every qubit contributes its partner mask)."""
    rng = _rng("rot:" + name)
    seen, out = set(), []
    for q in qubits:
        k = int(rng.choice(kinds))
        if pair_first and q not in seen:
            k = int(rng.choice((RX, RY)))
        seen.add(q)
        out.append((k, int(q), -1))
    return out


# ---- circuit cases ----------------------------------------------------------------------------------------------------
def flip_circuit(kind, code):
    """Slots e_A, e_B, e_C, then an op of ``kind`` whose partner mask is combination ``code`` of them, RZs in between."""
    head = [(RX, A, -1), (RY, B, -1), (RX, C, -1), (RZ, B, -1)]
    if kind == RYY:
        dep = {1: [(CX, A, B), (RYY, A, B)], 2: [(CX, B, A), (RYY, B, A)], 4: [(CX, C, A), (RYY, C, A)],
               3: [(RYY, A, B)], 5: [(RYY, A, C)], 6: [(RYY, B, C)], 7: [(CX, A, C), (RYY, A, B)]}[code]
    else:
        dep = {1: [(kind, A, -1)], 2: [(kind, B, -1)], 4: [(kind, C, -1)],
               3: [(CX, A, B), (kind, A, -1)], 5: [(CX, A, C), (kind, A, -1)], 6: [(CX, B, C), (kind, B, -1)],
               7: [(CX, A, B), (CX, A, C), (kind, A, -1)]}[code]
    return head + dep + [(RZ, A, -1)]


def code3_twice():
    """RX a, RX b, CNOT(a, b), RX a, RY a: the fourth and fifth masks are e_a ^ e_b; RX a, RX b and the first dependent
    op are three consecutive ops (one sweep of the gradient's backward kernel at the right alignment)."""
    return [(RX, A, -1), (RX, B, -1), (CX, A, B), (RX, A, -1), (RZ, B, -1), (RY, A, -1), (RZ, A, -1)]


def xor3_aligned4():
    """Four consecutive pair ops, the fourth's mask the XOR of the other three: flip code 7 of an aligned group of
    four of the untiled kernels (k_s_opk<4>), and of a chunk of the tiled ones."""
    return [(RX, A, -1), (RY, B, -1), (RX, C, -1), (CX, A, B), (CX, A, C), (RY, A, -1), (RZ, C, -1), (RX, 3, -1)]


def sweep3_circuit(kind):
    """Three times "slot, slot, an op of ``kind`` whose mask is the XOR of the two", at op offsets 0, 4 and 8: behind 0,
    1 or 2 extra ops one of the three triples is an aligned group of the three-op sweeps of the gradient's backward
    kernel (flip code 3 there); the first triple also lies in an aligned group of four of the untiled kernels."""
    out = []
    for a, b in ((A, B), (C, 4), (7, 12)):
        dep = [(RYY, a, b)] if kind == RYY else [(CX, a, b), (kind, a, -1)]
        out += [(RX, a, -1), (RY, b, -1)] + dep + [(RZ, b, -1)]
    return out[:-1]


def pass_circuit(n, last_qubit, rounds=1, name="pass"):
    """Behind a CNOT ladder: rotations on qubits 3 .. last_qubit, ``rounds`` times over."""
    qs = list(range(3, last_qubit + 1)) * rounds
    return ladder(n) + rotations(qs, "%s:%d:%d:%d" % (name, n, last_qubit, rounds))


def two_pass_circuit(n=N):
    """Certified two passes: nine independent partner masks behind a few CNOTs."""
    return [(CX, 3, 7), (CX, 12, 4), (CX, 0, 9)] + rotations(range(3, 12), "two_pass:%d" % n) + [(CX, 5, 13), (RZ, 13, -1)]


def outside_span_hamiltonian():
    """Every X mask has a bit among qubits 11..13 (outside the span of a pass on e_0..e_10) + a diagonal part."""
    rng = _rng("outside")
    terms = [(0, int(rng.integers(1 << N)), float(rng.normal())) for _ in range(3)]
    for x in (1 << 11, (1 << 12) | (1 << 3), (1 << 13) | (1 << 11) | 1, (1 << 12) | (1 << 13)):
        terms.append((x, int(rng.integers(1 << N)), float(rng.normal())))
    return ham_arrays(terms)


def few_groups_hamiltonian():
    """Five pair groups and no diagonal part: a last pass with two circuit masks has room for all of them."""
    rng = _rng("few")
    xs = [(1 << 4) | (1 << 9), 1 << 12, (1 << 6) | (1 << 7) | (1 << 13), (1 << 3) | 1, (1 << 10) | (1 << 4)]
    return ham_arrays([(x, int(rng.integers(1 << N)), float(rng.normal())) for x in xs for _ in range(2)])


def circuit_cases():
    """-> [(name, group, n, gates, ham)]"""
    out = []
    for kind in (RX, RY, RYY):
        for code in range(1, 8):
            out.append(("flip_%s_%d" % (KIND_NAME[kind], code), "flip", N, flip_circuit(kind, code), H12()))
    out.append(("flip_code3_twice", "flip", N, code3_twice(), H12()))
    out.append(("flip_xor3_aligned4", "flip", N, xor3_aligned4(), H12()))
    for kind in (RX, RY, RYY):
        out.append(("sweep3_%s" % KIND_NAME[kind], "flip", N, sweep3_circuit(kind), H12()))
    # chunk limits
    out.append(("chunk_rz7", "chunk", N, [(RZ, q, -1) for q in (0, 5, 13, 5, 9, 2, 7)], H12()))
    out.append(("chunk_rz13", "chunk", N, [(RZ, q, -1) for q in (1, 4, 4, 12, 3, 0, 13, 8, 8, 6, 2, 10, 11)], H12()))
    out.append(("chunk_pair3_rz4", "chunk", N, [(RX, 4, -1), (RY, 6, -1), (RX, 9, -1)] + [(RZ, q, -1) for q in (6, 1, 12, 9)], H12()))
    out.append(("chunk_pair4", "chunk", N, [(RY, 4, -1), (RX, 7, -1), (RY, 10, -1), (RX, 13, -1)], H12()))
    out.append(("chunk_pair2", "chunk", N, [(RX, 6, -1), (RZ, 6, -1), (RY, 12, -1)], H12()))
    # masks inside the tile's low bits
    out.append(("low_qubits", "low", N, [(RX, 0, -1), (RY, 1, -1), (RX, 2, -1), (RZ, 1, -1), (RY, 0, -1), (RX, 1, -1),
                                          (RY, 2, -1), (RZ, 0, -1), (RX, 2, -1), (RY, 1, -1)], H12()))
    # pass limits, behind CNOT ladders
    out.append(("pass_full_basis", "pass", N, pass_circuit(N, 10, rounds=2), H12()))
    out.append(("pass_two", "pass", N, pass_circuit(N, 10, rounds=2) + [(RY, 11, -1)], H12()))
    out.append(("pass_three", "pass", N, pass_circuit(N, 13, rounds=2), H12()))
    out.append(("pass_three_n16", "pass", 16, pass_circuit(16, 15, rounds=2), H12(16)))
    # degenerate circuits
    rng = _rng("cnot40")
    c = rng.integers(0, N, 40)
    t = (c + 1 + rng.integers(0, N - 1, 40)) % N
    out.append(("empty_circuit", "degenerate", N, [], H12()))
    out.append(("cnot40", "degenerate", N, [(CX, int(a), int(b)) for a, b in zip(c, t)], H12()))
    out.append(("one_qubit_300", "degenerate", N, rotations([5] * 300, "one_qubit"), H12()))
    out.append(("last_pass_full", "degenerate", N, rotations(range(3, 11), "last_full"), outside_span_hamiltonian()))
    out.append(("last_pass_room_for_all", "degenerate", N, [(RX, 5, -1), (RY, 8, -1)], few_groups_hamiltonian()))
    # SU(4) ops: RXX / RYY as slot ops, RZZ as a diagonal rider, RXX / RX / RYY as dependent ops
    out.append(("su4_slots_and_rider", "su4", N, [(RXX, 4, 9), (RYY, 6, 12), (RZZ, 4, 6), (RY, 4, -1), (RYY, 4, 9), (RX, 9, -1)], H12()))
    out.append(("su4_dependent", "su4", N, [(RX, A, -1), (RYY, B, C), (RZZ, A, C), (RY, B, -1), (RXX, A, B), (RYY, A, C)], H12()))
    return out


# ---- Hamiltonian cases ------------------------------------------------------------------------------------------------
def bond(a, b, w, rel=1.0, zstring=True):
    """X Z..Z X + rel Y Z..Z Y on qubits a < b (coefficients of the Pauli strings)."""
    x = (1 << a) | (1 << b)
    zs = sum(1 << k for k in range(a + 1, b)) if zstring else 0
    return [(x, zs, w), (x, zs | x, rel * w)]


def hamiltonian_cases():
    """-> [(name, n, ham, backgrounds)]; backgrounds: the circuits the case runs behind ("empty", "two_pass").  Every
    case draws from a generator seeded by its own name: editing one case leaves the others as they are."""
    both = ("empty", "two_pass")
    out = []

    class Draw:
        def __init__(self, name):
            self.rng = _rng("ham:" + name)

        def z(self):
            return int(self.rng.integers(1 << N))

        def w(self):
            return float(self.rng.normal())

        def even(self, x):      # a Z mask with an even overlap with x: a real weight
            z = self.z()
            return z ^ (x & -x) if bin(x & z).count("1") % 2 else z

        def odd(self, x):       # an odd number of Y factors: an imaginary weight
            return self.even(x) ^ (x & -x)

        def masks(self, count):
            xs = []
            while len(xs) < count:
                x = int(self.rng.integers(1, 1 << N))
                if x not in xs:
                    xs.append(x)
            return xs

    def case(name, build, backgrounds=both):
        out.append((name, N, ham_arrays(build(Draw(name))), backgrounds))

    case("ham_empty", lambda d: [])
    case("ham_identity", lambda d: [(0, 0, 0.75)])
    # behind an empty circuit the diagonal group's pass is e_0..e_10: the class of a term is bits 8..10 of its Z mask
    case("ham_diag_one_class", lambda d: [(0, (d.z() & ~0x700) | 0x300, d.w()) for _ in range(5)])
    case("ham_diag_eight_classes", lambda d: [(0, (d.z() & ~0x700) | (cls << 8), d.w()) for cls in range(8) for _ in range(1 + cls % 2)])
    case("ham_no_diagonal", lambda d: [(x, d.z(), d.w()) for x in (0b10010000, 1 << 13, 0b1100000001)])

    # pair groups of 1, 2, 3 and 4 terms with real weights; five groups in the pass, and six
    def by_terms(d, extra):
        groups = ((1 << 5, 1), (0b11 << 8, 2), ((1 << 12) | 1, 3), ((1 << 4) | (1 << 13), 4), (1 << 7, 1)) + extra
        return [(x, d.even(x), d.w()) for x, nt in groups for _ in range(nt)]
    case("ham_terms_1_2_3_odd_groups", lambda d: by_terms(d, ()))
    case("ham_terms_even_groups", lambda d: by_terms(d, (((1 << 6) | (1 << 2), 1),)))

    # imaginary weights: six groups whose masks fit the fused pass and ten more that do not
    def imaginary(d):
        xs_in = [1 << q for q in (3, 4, 5, 6, 7, 8)]
        xs_out = [(1 << q) | (1 << ((q + 5) % 11 + 3)) | int(d.rng.integers(8)) for q in range(3, 13)]
        return ([(x, d.odd(x), d.w()) for x in xs_in for _ in range(2)] + [(x, d.odd(x), d.w()) for x in xs_out] +
                [(x, d.even(x), d.w()) for x in xs_out[:4]])
    case("ham_imaginary_fused_and_own", imaginary)

    # half groups: chain bonds, both relative signs, bonds into the tile's low qubits
    def chain(d):
        terms = []
        for a, rel in zip(range(3, 13), (1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, -1.0, 1.0)):
            terms += bond(a, a + 1, d.w(), rel=rel)
        return terms + bond(0, 6, d.w()) + bond(2, 9, d.w(), rel=-1.0) + bond(4, 11, d.w())
    case("ham_half_chain", chain)
    # two-term groups that must not become half groups
    case("ham_half_refused_unequal", lambda d: bond(4, 5, d.w(), rel=0.5) + bond(7, 10, d.w(), rel=-2.0))
    case("ham_half_refused_zero", lambda d: bond(4, 5, 0.0) + bond(6, 12, d.w()))
    x49 = (1 << 4) | (1 << 9)
    case("ham_half_refused_imaginary", lambda d: [(x49, 1 << 4, d.w()), (x49, 1 << 9, d.w())] + bond(6, 12, d.w()))
    # XX + YY on disjoint pairs: z1 ^ z2 = x meets no other basis vector of a pass that holds only such masks
    case("ham_half_refused_czd0", lambda d: [t for a in (4, 6, 8, 10, 12) for t in bond(a, a + 1, d.w(), rel=(1.0, -1.0)[(a // 2) % 2])])
    # many independent masks: three energy passes and more, k_t_energy's own passes with odd and with even group counts
    case("ham_many_passes", lambda d: [(0, d.z(), d.w()), (0, d.z(), d.w())] + [(x, d.even(x), d.w()) for x in d.masks(40)])
    # 217 X-mask groups: the last count on the tiled kernels; 218: the first on the untiled ones (stream_tiled)
    case("ham_217_groups", lambda d: [(x, d.even(x), d.w()) for x in d.masks(217)], ("empty",))
    case("ham_218_groups", lambda d: [(x, d.even(x), d.w()) for x in d.masks(218)], ("empty",))
    return out


def background(name, n=N):
    return {"empty": [], "two_pass": two_pass_circuit(n)}[name]
