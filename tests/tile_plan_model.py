"""Host restatement of the decisions of the streaming path's two device planners, k_t_plan_ops and k_t_plan_energy
(csrc/vqe_tile.h), behind k_s_compile and k_s_terms (csrc/vqe_stream.h): noiseless gate list + Pauli sum -> which
passes, chunks, flip codes, fused groups, energy passes and group paths the kernels will run.

Pure Python, no GPU.  It computes no amplitude and is never the reference for a value - the oracle is.  Its one job is
to say which planner branch an input reaches, so that a GPU case certifiably tests what its name says
(tests/stream_cases.py, tests/test_tile_plan_cpu.py).  Where the model and the device disagree no value test fails;
the model is then the one to fix.

The tile constants are restated here and compared with csrc/vqe_tile.h by the CPU test (``parse_constants``): a
retuned tile size makes the model fail instead of going stale."""
import os
import re

# csrc/vqe_tile.h
kTileBits = 11
kTileLow = 3
kETileBits = 11
kETileLow = 4
kChunkOps = 6
kMaxEnergyPasses = 32
kTileK = kTileBits - 8          # slots of a chunk
kETileFree = kETileBits - kETileLow
kMaxTiledTerms = 4096           # stream_tiled (csrc/vqe_stream.h)

# gate kinds of the C ABI (include/vqe_hip.h) and op kinds of csrc/vqe_device.h
G_CNOT, G_RX, G_RY, G_RZ, G_RXX, G_RYY, G_RZZ = 0, 1, 2, 3, 6, 7, 8
OP_RX, OP_RY, OP_RZ, OP_RYY = 1, 2, 3, 7
OP_NAME = {OP_RX: "rx", OP_RY: "ry", OP_RZ: "rz", OP_RYY: "ryy"}

TILE_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensorrl-qas_amd", "csrc", "vqe_tile.h")


def parse_constants(path=TILE_HEADER):
    """The constants as csrc/vqe_tile.h defines them (the #define defaults and the two plain constexpr ints)."""
    text = open(path).read()

    def macro(name):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m, name
        return int(m.group(1))

    def const(name):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, name
        return int(m.group(1))

    return {"kTileBits": macro("VQE_TILE_BITS"), "kTileLow": macro("VQE_TILE_LOW"), "kETileLow": macro("VQE_ETILE_LOW"),
            "kETileBits": macro("VQE_ETILE_BITS"), "kChunkOps": const("kChunkOps"),
            "kMaxEnergyPasses": const("kMaxEnergyPasses")}


def model_constants():
    return {"kTileBits": kTileBits, "kTileLow": kTileLow, "kETileLow": kETileLow, "kETileBits": kETileBits,
            "kChunkOps": kChunkOps, "kMaxEnergyPasses": kMaxEnergyPasses}


def parity(x):
    return bin(x).count("1") & 1


def top_bit(x):
    return x.bit_length() - 1


def op_is_pair(kind):
    return kind in (OP_RX, OP_RY, OP_RYY)


# ---- k_s_compile (noiseless) and k_s_terms ----------------------------------------------------------------------------
class Op:
    __slots__ = ("kind", "xm", "zm", "gate")

    def __init__(self, kind, xm, zm, gate):
        self.kind, self.xm, self.zm, self.gate = kind, xm, zm, gate


def compile_gates(n, gates):
    """gates: (kind, q0, q1) in order of application -> (ops, xm, zm).  CNOTs only update the frame: xm[q] is the
    physical partner mask of logical qubit q, zm[q] its physical sign mask; every rotation is one op in that frame."""
    xm = [1 << q for q in range(n)]
    zm = [1 << q for q in range(n)]
    ops = []
    for i, (kind, a, b) in enumerate(gates):
        if kind == G_CNOT:
            zm[b] ^= zm[a]
            xm[a] ^= xm[b]
        elif kind in (G_RX, G_RY, G_RZ):
            ops.append(Op(kind, xm[a], zm[a], i))
        elif kind in (G_RXX, G_RYY, G_RZZ):
            ops.append(Op({G_RXX: OP_RX, G_RYY: OP_RYY, G_RZZ: OP_RZ}[kind], xm[a] ^ xm[b], zm[a] ^ zm[b], i))
        else:
            raise ValueError("the model restates noiseless gate lists only")
    return ops, xm, zm


def group_hamiltonian(xmask, zmask, coeff):
    """ham_from_paulis + the streaming group list (csrc/ham_layout.h): groups by X mask in order of first appearance,
    terms in input order, weight c i^{#Y} as (real, imaginary)."""
    index, groups = {}, []
    for x, z, c in zip(xmask, zmask, coeff):
        x, z, c = int(x), int(z), float(c)
        ny = bin(x & z).count("1") & 3
        wr = c if ny == 0 else (-c if ny == 2 else 0.0)
        wi = c if ny == 1 else (-c if ny == 3 else 0.0)
        if x not in index:
            index[x] = len(groups)
            groups.append((x, []))
        groups[index[x]][1].append((z, wr, wi))
    return groups


def physical_masks(n, groups, xm, zm):
    """k_s_terms: x' = XOR of xm[q] over the bits of x, z' likewise with zm (the sign (-1)^{z.c} is +1 without noise)."""
    def move(v, cols):
        out = 0
        for q in range(n):
            if (v >> q) & 1:
                out ^= cols[q]
        return out
    return [(move(x, xm), [(move(z, zm), wr, wi) for z, wr, wi in terms]) for x, terms in groups]


# ---- TileBasis --------------------------------------------------------------------------------------------------------
class TileBasis:
    def __init__(self, low, bits):
        self.low, self.bits = low, bits
        self.reset()

    def reset(self):
        self.v = [1 << i for i in range(self.low)]
        self.piv = list(range(self.low))

    @property
    def dim(self):
        return len(self.v)

    def reduce(self, x):
        for v, p in zip(self.v, self.piv):
            if (x >> p) & 1:
                x ^= v
        return x

    def add(self, r):
        p = top_bit(r)
        self.v = [v ^ r if (v >> p) & 1 else v for v in self.v]
        self.v.append(r)
        self.piv.append(p)

    def fill(self, n):
        for q in range(self.low, n):
            if self.dim >= self.bits:
                break
            r = self.reduce(1 << q)
            if r:
                self.add(r)

    def sort(self):
        order = sorted(range(self.dim), key=lambda i: self.piv[i])
        self.v = [self.v[i] for i in order]
        self.piv = [self.piv[i] for i in order]

    def coords(self, x):
        return sum(((x >> p) & 1) << i for i, p in enumerate(self.piv))

    def zcoords(self, z):
        return sum(parity(v & z) << i for i, v in enumerate(self.v))

    def copy(self):
        b = TileBasis(self.low, self.bits)
        b.v, b.piv = list(self.v), list(self.piv)
        return b


# ---- k_t_plan_ops -----------------------------------------------------------------------------------------------------
def plan_chunk(ops, cx, o, end):
    """The chunk that starts at op o of a pass ending at ``end``, in tile coordinates."""
    red, hbit, g = [], [], []

    def reduce(x):
        for r, h in zip(red, hbit):
            if (x >> h) & 1:
                x ^= r
        return x

    def push(x):
        h = top_bit(x)
        for i in range(len(red)):
            if (red[i] >> h) & 1:
                red[i] ^= x
        red.append(x)
        hbit.append(h)

    cnt, slot_of, ended = 0, [], "end"
    while o + cnt < end:
        if cnt == kChunkOps:
            ended = "cap"
            break
        s = -1
        if op_is_pair(ops[o + cnt].kind):
            r = reduce(cx[o + cnt])
            if r:
                if len(g) == kTileK:
                    ended = "fourth"        # a fourth independent mask: the next chunk
                    break
                push(r)
                s = len(g)
                g.append(cx[o + cnt])
        slot_of.append(s)
        cnt += 1
    nslots = len(g)
    q = 0
    while len(g) < kTileK:                  # fillers for the unused slots
        while reduce(1 << q) == 0:
            q += 1
        push(reduce(1 << q))
        g.append(1 << q)
        q += 1
    flips, dependent = [], []
    for j in range(cnt):
        op = ops[o + j]
        flip = 0
        if op_is_pair(op.kind):
            if slot_of[j] >= 0:
                flip = 1 << slot_of[j]
            else:
                for f in range(1, 1 << kTileK):
                    x = 0
                    for i in range(kTileK):
                        if (f >> i) & 1:
                            x ^= g[i]
                    if x == cx[o + j]:
                        flip = f
                assert flip, "a dependent mask lies in the span of the slots"
                dependent.append((op.kind, flip))
        flips.append(flip)
    return {"begin": o, "count": cnt, "slots": nslots, "fillers": kTileK - nslots,
            "pair_ops": sum(op_is_pair(ops[o + j].kind) for j in range(cnt)), "flips": flips, "dependent": dependent,
            "ended": ended, "slot_masks": g,
            "low_pair": any(op_is_pair(ops[o + j].kind) and ops[o + j].xm < (1 << kTileLow) for j in range(cnt))}


def plan_ops(n, ops, gxp=None):
    """-> passes: dicts with the closed basis (TileBasis, sorted), begin, end, the chunks, and for the last pass the
    number of basis vectors that came from group masks.  ``gxp``: the physical X masks of the groups (the fused plan)."""
    passes = []
    B = TileBasis(kTileLow, kTileBits)
    state = {"begin": 0}

    def close(end, last=False):
        taken = 0
        if last and gxp is not None:
            for x in gxp:
                if B.dim >= kTileBits:
                    break
                r = B.reduce(x)
                if r:
                    B.add(r)
                    taken += 1
        dim_before_fill = B.dim
        B.fill(n)
        B.sort()
        basis = B.copy()
        begin = state["begin"]
        cx = {o: (basis.coords(ops[o].xm) if op_is_pair(ops[o].kind) else 0) for o in range(begin, end)}
        chunks, o = [], begin
        while o < end:
            c = plan_chunk(ops, cx, o, end)
            chunks.append(c)
            o += c["count"]
        passes.append({"basis": basis, "begin": begin, "end": end, "chunks": chunks, "group_vectors": taken,
                       "dim_before_fill": dim_before_fill})

    for o, op in enumerate(ops):
        if not op_is_pair(op.kind):
            continue                        # diagonal ops fit every tile
        r = B.reduce(op.xm)
        if not r:
            continue
        if B.dim < kTileBits:
            B.add(r)
            continue
        close(o)                            # the (kTileBits - kTileLow + 1)-th independent mask closes the pass
        state["begin"] = o
        B.reset()
        B.add(B.reduce(op.xm))
    close(len(ops), True)                   # (a stream without ops still gets its copy pass)
    return passes


# ---- the aligned K-op sweeps of k_s_opk<4> (untiled forward kernels) and k_sg_back<3> (streaming gradient) -------------
def sweep_flip_codes(ops, K):
    """Both kernels cut the op list into aligned groups [o, o + K), o = 0, K, 2K, ..: op j of a group owns slot j when
    its physical partner mask is independent of the slots before it, the other slots get filler unit vectors, and a
    dependent pair op gets the combination of slot masks that equals its mask.  -> per group the (kind, flip code) of
    its dependent ops; a code with one bit is "the same mask twice", a code with several the generic exchange."""
    out = []
    for o in range(0, len(ops), K):
        grp = ops[o:o + K]
        red, hbit, g, own = [], [], [0] * K, [False] * K

        def reduce(x):
            for r, h in zip(red, hbit):
                if (x >> h) & 1:
                    x ^= r
            return x

        def push(x):
            h = top_bit(x)
            for i in range(len(red)):
                if (red[i] >> h) & 1:
                    red[i] ^= x
            red.append(x)
            hbit.append(h)

        for j, op in enumerate(grp):
            if op_is_pair(op.kind):
                r = reduce(op.xm)
                if r:
                    push(r)
                    g[j], own[j] = op.xm, True
        q = 0
        for j in range(K):
            if not own[j]:
                while reduce(1 << q) == 0:
                    q += 1
                push(reduce(1 << q))
                g[j] = 1 << q
                q += 1
        dep = []
        for j, op in enumerate(grp):
            if op_is_pair(op.kind) and not own[j]:
                flip = 0
                for f in range(1, 1 << K):
                    x = 0
                    for i in range(K):
                        if (f >> i) & 1:
                            x ^= g[i]
                    if x == op.xm:
                        flip = f
                assert flip
                dep.append((op.kind, flip))
        out.append(dep)
    return out


# ---- k_t_plan_energy --------------------------------------------------------------------------------------------------
def plan_energy(n, pgroups, last_pass_basis=None):
    """pgroups: physical_masks() output.  ``last_pass_basis``: the sorted basis of the stream's last circuit pass (fused
    plan: it becomes pass 0 as it is) or None.  -> (passes, groups): passes are dicts {basis, groups (ids in the order
    they run), fused}; groups are dicts with the pass and the path the kernel takes."""
    fused = last_pass_basis is not None
    bases = []
    if fused:
        assert last_pass_basis.dim == kETileBits == kTileBits
        bases.append(last_pass_basis.copy())
    gpass = []
    for x, _ in pgroups:
        dst = -1
        for k in range(1 if (fused and x == 0) else 0, len(bases)):
            r = bases[k].reduce(x)
            if not r:
                dst = k
            elif bases[k].dim < kETileBits:
                bases[k].add(r)
                dst = k
            if dst >= 0:
                break
        if dst < 0:
            assert len(bases) < kMaxEnergyPasses, "the host bounds n_groups so that this cannot happen"
            b = TileBasis(kETileLow, kETileBits)
            r = b.reduce(x)
            if r:
                b.add(r)
            bases.append(b)
            dst = len(bases) - 1
        gpass.append(dst)
    if not bases:
        bases.append(TileBasis(kETileLow, kETileBits))      # a Hamiltonian shard without groups: one empty pass
    passes, groups = [], [None] * len(pgroups)
    for k, b in enumerate(bases):
        b.fill(n)
        b.sort()
        assert b.dim == kETileBits
        ids = [g for g in range(len(pgroups)) if gpass[g] == k]
        passes.append({"basis": b, "groups": ids, "fused": fused and k == 0})
        for g in ids:
            x, terms = pgroups[g]
            c = b.coords(x)
            info = {"pass": k, "fused": fused and k == 0, "terms": len(terms), "cx": c}
            czs = [b.zcoords(z) for z, _, _ in terms]
            imag = any(wi != 0.0 for _, _, wi in terms)
            if c == 0:
                info["path"] = "diagonal"
                info["classes"] = sorted({cz >> 8 for cz in czs})
            else:
                hb = top_bit(c)
                info["hb"] = hb
                info["imag"] = imag
                info["path"] = "general"
                info["refusal"] = None
                if len(terms) == 2:
                    w1, w2 = terms[0][1], terms[1][1]
                    czd = (czs[0] ^ czs[1]) & ~(1 << hb)
                    if imag:
                        info["refusal"] = "imaginary"
                    elif not (w1 == w2 or w1 == -w2):
                        info["refusal"] = "unequal"
                    elif w1 == 0.0:
                        info["refusal"] = "zero"
                    elif czd == 0:
                        info["refusal"] = "czd0"
                    else:
                        q = top_bit(czd)
                        info["path"] = "half"
                        info["q"] = q
                        info["q_below_hb"] = q < hb
                        info["opposite"] = w1 != w2
            groups[g] = info
    return passes, groups


def stream_tiled(n_groups, n_terms):
    """stream_tiled of csrc/vqe_stream.h without its environment switch: the tiled kernels serve this shard."""
    return (n_groups + kETileFree - 1) // kETileFree + 1 <= kMaxEnergyPasses and n_terms <= kMaxTiledTerms


# ---- summary ----------------------------------------------------------------------------------------------------------
def plan(n, gates, ham, fuse=True):
    """The whole plan of one stream: ops, circuit passes, energy passes, groups."""
    ops, xm, zm = compile_gates(n, gates)
    groups = group_hamiltonian(*ham)
    pgroups = physical_masks(n, groups, xm, zm)
    tiled = stream_tiled(len(groups), sum(len(t) for _, t in groups))
    out = {"n": n, "ops": ops, "tiled": tiled, "n_groups": len(groups), "pgroups": pgroups}
    if not tiled:
        return out
    out["passes"] = plan_ops(n, ops, [x for x, _ in pgroups] if fuse else None)
    out["epasses"], out["groups"] = plan_energy(n, pgroups, out["passes"][-1]["basis"] if fuse else None)
    return out


def summarize(n, gates, ham, fuse=True):
    """The plan of one stream in the terms the planner branches are named in: passes, chunks, flip codes, fused groups,
    energy passes, group paths, diagonal classes."""
    p = plan(n, gates, ham, fuse)
    s = {"tiled": p["tiled"], "n_ops": len(p["ops"]), "n_groups": p["n_groups"]}
    if not p["tiled"]:
        return s
    chunks = [c for ps in p["passes"] for c in ps["chunks"]]
    groups = p["groups"]
    pair_groups = [g for g in groups if g["path"] != "diagonal"]
    s.update({
        "passes": len(p["passes"]),
        "chunks": [{k: c[k] for k in ("count", "slots", "fillers", "pair_ops", "dependent", "ended", "low_pair")} for c in chunks],
        "dependent": sorted({d for c in chunks for d in c["dependent"]}),
        "last_pass_room": kTileBits - (p["passes"][-1]["dim_before_fill"] - p["passes"][-1]["group_vectors"]),
        "fused_groups": sum(g["fused"] for g in groups),
        "pair_groups": len(pair_groups),
        # passes that hold no group run nothing (an empty Hamiltonian's one pass, a fused pass no group closes in)
        "energy_passes": len(p["epasses"]),
        "own_passes": sum(1 for e in p["epasses"] if not e["fused"] and e["groups"]),
        "pass_group_counts": [len(e["groups"]) for e in p["epasses"]],
        "own_pass_group_counts": [len(e["groups"]) for e in p["epasses"] if not e["fused"] and e["groups"]],
        "group_paths": [_path_name(g) for g in groups],
        "diag_classes": next((g["classes"] for g in groups if g["path"] == "diagonal"), None),
    })
    return s


def _path_name(g):
    """diagonal | half:{equal,opposite}:{q<hb,q>hb} | general:{1,2,3+}[:imag][:refused-<why>], suffixed @fused / @own"""
    where = "@fused" if g["fused"] else "@own"
    if g["path"] == "diagonal":
        return "diagonal" + where
    if g["path"] == "half":
        return "half:%s:%s%s" % ("opposite" if g["opposite"] else "equal", "q<hb" if g["q_below_hb"] else "q>hb", where)
    name = "general:%s" % (g["terms"] if g["terms"] < 3 else "3+")
    if g["imag"]:
        name += ":imag"
    if g["refusal"]:
        name += ":refused-" + g["refusal"]
    return name + where
