"""Multi-GPU use of the engine: one process per GPU (torch.distributed, backend "nccl" =
RCCL over xGMI on ROCm; "gloo" in CPU tests).

Two ways the path shards:
* parallel environments / RL seeds - replicas, no data-path collective (``env_shard``);
* Pauli-term sharding of <psi|H|psi> - every rank applies the same circuit to its own copy
  of the state and evaluates a disjoint set of X-mask groups; ONE all-reduce of the partial
  energies (8 bytes per evaluation) completes each batch of evaluations.
The reference has no counterpart (single process)."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from .engine import HostCobyla


def dist_env():
    """(rank, world_size, local_rank) from the launcher's environment (torchrun)."""
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")),
            int(os.environ.get("LOCAL_RANK", "0")))


def env_shard(num_envs_total: int, rank: int, world: int) -> range:
    """Contiguous block of environment ids owned by ``rank`` (sizes differ by at most 1)."""
    base, rem = divmod(num_envs_total, world)
    lo = rank * base + min(rank, rem)
    return range(lo, lo + base + (1 if rank < rem else 0))


def term_owner(n_qubits: int, xmask, world: int) -> np.ndarray:
    """Rank owning each Pauli term under vqe_set_term_shard(rank, world) (host only)."""
    x = np.ascontiguousarray(xmask, np.uint64)
    out = np.zeros(x.size, np.int32)
    rc = _lib.load().vqe_term_owner(int(n_qubits), int(x.size), x.ctypes.data_as(_lib.c_u64p), int(world),
                                    out.ctypes.data_as(_lib.c_i32p))
    if rc:
        raise _lib.VQEError(f"vqe_term_owner failed ({rc})")
    return out


def allreduce_sum(values, group=None):
    """Sum a float64 tensor (or array) of partial energies over all ranks, in place.

    Device tensors go to RCCL as they are (backend "nccl"); host values under RCCL travel through this rank's
    GPU.  Under gloo (CPU tests, the two-ranks-on-one-GPU test) a device tensor is summed through a host copy:
    gloo's own device path (pinned staging buffers filled by its worker threads) is never entered."""
    import torch
    import torch.distributed as dist
    t = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values, np.float64))
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        nccl = dist.get_backend(group) == "nccl"
        if t.is_cuda != nccl:
            d = t.to(torch.device("cuda", torch.cuda.current_device())) if nccl else t.cpu()
            dist.all_reduce(d, op=dist.ReduceOp.SUM, group=group)
            t.copy_(d)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def sharded_minimize(partial_energy, x0, rhobeg=1.0, rhoend=1e-4, maxfun=1000, group=None):
    """COBYLA where every evaluation is ``allreduce_sum(partial_energy(x))``.  All ranks run
    the same ask/tell sequence on bit-identical reduced energies, so they stay in lock-step
    without broadcasting x.  ``partial_energy(x) -> float`` (this rank's share)."""
    opt = HostCobyla(x0, rhobeg, rhoend, maxfun)
    while True:
        x = opt.ask()
        if x is None:
            break
        e = allreduce_sum(np.array([partial_energy(x)], np.float64), group)
        opt.tell(float(e[0]))
    return opt.result()


class TermShardedEngine:
    """An engine that owns ``rank``'s share of the Pauli terms; ``energies()`` returns the
    all-reduced energies of the resident batch as a device tensor."""

    def __init__(self, engine, rank: int, world: int, device, by_amplitude: bool | None = None):
        import torch
        self.engine, self.rank, self.world = engine, rank, world
        self.device = torch.device(device)
        # n >= 14: slice the amplitude range (1/world of the sweep per rank, perfectly
        # balanced); n <= 13: a workgroup holds the whole state, so split the X-mask groups
        if by_amplitude is None:
            by_amplitude = not engine.device_info()["lds_path"]
        if by_amplitude:
            engine.set_amplitude_shard(rank, world)
        else:
            engine.set_term_shard(rank, world)
        # ONE stream for the engine's launches, the device-to-device copy and the collective: a torch stream of
        # this object's own that the handle is told to issue on (vqe_set_stream), so inside energies() plain stream
        # order is all the ordering there is; the caller's current stream is ordered against it once on the way
        # in and once on the way out, with torch's own wait_stream on torch's own streams.  (torch's DEFAULT stream
        # cannot be handed to the handle: its pointer is NULL, which vqe_set_stream reads as "your own stream" -
        # a non-blocking one that the default stream does not order against.  Round 2 wrapped the handle's stream
        # in torch.cuda.ExternalStream instead; that code is gone.)
        with torch.cuda.device(self.device):
            self._stream = torch.cuda.Stream(device=self.device)
        engine.set_stream(self._stream.cuda_stream)
        self._buf = None

    def close(self):
        """Give the handle its own stream back (after draining this object's) and drop the result buffer."""
        if self.engine is not None:
            self._stream.synchronize()
            self.engine.set_stream(None)
            self.engine, self._buf = None, None

    def energies(self, batch: int):
        import torch
        cur = torch.cuda.current_stream(self.device)
        self._stream.wait_stream(cur)             # whatever the caller still does with the previous result
        with torch.cuda.stream(self._stream):
            if self._buf is None or self._buf.numel() != batch:
                self._buf = torch.zeros(batch, dtype=torch.float64, device=self.device)
            self.engine.batch_run_energy()
            self.engine.batch_copy_energy(self._buf.data_ptr())
            out = allreduce_sum(self._buf)
        cur.wait_stream(self._stream)             # the caller reads the sum on its own stream
        out.record_stream(cur)
        return out

    def partial_energies(self):
        """This rank's share of the energies of the resident batch (host array, not reduced)."""
        self.engine.batch_run_energy()
        return self.engine.batch_fetch(want_x=False)[1]

    def minimize(self, circuit, x0, rhobeg=1.0, rhoend=1e-4, maxfun=1000):
        """Lock-step COBYLA over all ranks on the all-reduced energy (``sharded_minimize`` does
        the reduction: ``partial`` must return this rank's share only)."""
        def partial(x):
            self.engine.batch_load([circuit], [x])
            return float(self.partial_energies()[0])
        return sharded_minimize(partial, x0, rhobeg, rhoend, maxfun)


def fit_restarts_sharded(fit_shard, n_restarts_total: int, group=None):
    """Random restarts of the MPS -> PQC fit spread over the ranks (independent units, replicas
    only): every rank fits its contiguous share of the restart ids and ONE all-gather of the
    best losses (8 bytes per rank) picks the winner, whose gates are broadcast.

    ``fit_shard(restart_ids: range) -> (best_val: float, gates: ndarray[G,4,4] complex)`` runs
    this rank's restarts (on the GPU: ``dmrg_to_qc.mps_to_qc(..., n_restarts=len(ids))`` with a
    generator seeded per restart id, so the result does not depend on the world size).
    Returns ``(best_val, gates, owner_rank)``, identical on all ranks; ties go to the lowest rank."""
    import torch
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank(group) if on else 0
    world = dist.get_world_size(group) if on else 1
    ids = env_shard(n_restarts_total, rank, world)
    val, gates = fit_shard(ids) if len(ids) else (float("inf"), None)
    if world == 1:
        return float(val), gates, 0
    # RCCL moves device memory only: the few bytes exchanged live on this rank's GPU under "nccl"
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    vals = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
    dist.all_gather(vals, torch.tensor([float(val)], dtype=torch.float64, device=dev), group=group)
    owner = int(np.argmin([float(v[0]) for v in vals]))
    shape = torch.tensor(list(np.shape(gates)) if rank == owner else [0, 0, 0], dtype=torch.int64, device=dev)
    dist.broadcast(shape, src=owner, group=group)
    buf = torch.zeros(tuple(int(s) for s in shape.tolist()) + (2,), dtype=torch.float64, device=dev)
    if rank == owner:
        buf.copy_(torch.view_as_real(torch.as_tensor(np.ascontiguousarray(gates, np.complex128))))
    dist.broadcast(buf, src=owner, group=group)
    return float(vals[owner][0]), torch.view_as_complex(buf.cpu()).numpy().copy(), owner


# ----------------------------------------------------------------------------------------------------------------
# Amplitude-sharded STATES: a register of n qubits over world = 2^g ranks, 2^(n-g) amplitudes
# each.  The top g positions of the physical index are the rank; a logical qubit sits at a position that the planner
# tracks (pos[q]).  A gate whose qubits all sit at local positions needs no communication: a rank's shard is the
# "state" of an (n-g)-qubit handle of the engine (vqe_set_init_state_dev / vqe_get_state_dev: it never leaves the GPU).
# A gate - or the X / Y factor of a Pauli term - on a qubit at a rank position is preceded by a pairwise HALF-SHARD
# EXCHANGE that swaps that position with a local one (rank r keeps the half of its shard whose local bit equals its
# rank bit and trades the other half with rank r ^ bit: 2^(n-g-1) amplitudes each way, one xGMI link per pair); Z
# factors on rank positions are signs.  The reference has no counterpart (single process; its 2^n x 2^n matrix stops
# it at 13 qubits, environments/VQAs/VQE_qulacs_TN_notin_RL.py:86).
# Status: the planner and the executor below are exercised by tests (gloo world 2 / 4 / 8 on the CPU with a CPU stand-in
# as the local backend; all shards on ONE GPU with device-to-device copies as the exchange; two processes on one GPU
# with CUDA shards, gloo, the halves travelling through the host); no run on several GPUs exists yet, so there is no
# scaling curve for it.
# Streams: a backend that works on a stream of its own offers exchange_context(); the exchanges run under it, in plain
# stream order with the backend's copies (tests/test_stream_order_gpu.py delays either side by 30 ms).
def _log2_exact(v: int) -> int:
    g = int(v).bit_length() - 1
    if v < 1 or (1 << g) != v:
        raise ValueError("world size of amplitude-sharded states must be a power of two")
    return g


class ShardStep:
    """One step of a plan: ``kind`` = "gates" (``items`` = gate indices, all local under ``pos``), "energy" (``items`` =
    term indices whose X support is local under ``pos``) or "swap" (``rank_bit`` <-> local position ``local_pos``)."""
    __slots__ = ("kind", "items", "pos", "rank_bit", "local_pos")

    def __init__(self, kind, items=None, pos=None, rank_bit=-1, local_pos=-1):
        self.kind, self.items, self.pos, self.rank_bit, self.local_pos = kind, items, pos, rank_bit, local_pos


def plan_amplitude_sharding(n: int, world: int, kind, q0, q1, xmask):
    """Partition / exchange schedule for one circuit followed by the expectation sum of a Pauli Hamiltonian.

    Greedy with look-ahead: a qubit is brought to a local position only when a gate (or the X support of a term)
    needs it there, and the local qubit that gives way is the one whose next use lies farthest ahead.  Returns the
    list of steps and the number of exchanges."""
    g = _log2_exact(world)
    nl = n - g
    if nl < 1:
        raise ValueError("more ranks than amplitudes pairs")
    kind, q0, q1 = (np.asarray(a).astype(np.int64) for a in (kind, q0, q1))
    G = kind.size
    if np.any(kind > 5):      # RXX / RYY / RZZ (engine.GATE_RXX..GATE_RZZ): a rank-bit qubit of such a gate has no local form here
        raise NotImplementedError("amplitude sharding does not take RXX / RYY / RZZ gates")
    qubits = [[int(q0[i])] + ([int(q1[i])] if kind[i] in (0, 5) else []) for i in range(G)]
    supports = [[q for q in range(n) if (int(x) >> q) & 1] for x in xmask]
    if any(len(s) > nl for s in supports) or any(len(s) > nl for s in qubits):
        raise ValueError("a gate or Pauli term touches more qubits than a shard holds")
    pos = list(range(n))
    steps, swaps = [], 0

    def next_use(q, after):
        for j in range(after, G):
            if q in qubits[j]:
                return j
        # after the circuit: qubits that the Hamiltonian flips are wanted again, the others never
        return G + (0 if any(q in s for s in supports) else 1)

    def bring_local(q, keep, after):
        nonlocal swaps
        cand = [v for v in range(n) if pos[v] < nl and v not in keep]
        victim = max(cand, key=lambda v: (next_use(v, after), -v))
        steps.append(ShardStep("swap", rank_bit=pos[q] - nl, local_pos=pos[victim]))
        pos[q], pos[victim] = pos[victim], pos[q]
        swaps += 1

    cur = []
    for i in range(G):
        need = [q for q in qubits[i] if pos[q] >= nl]
        if need:
            if cur:
                steps.append(ShardStep("gates", items=cur, pos=list(pos)))
                cur = []
            for q in need:
                bring_local(q, qubits[i], i + 1)
        cur.append(i)
    if cur:
        steps.append(ShardStep("gates", items=cur, pos=list(pos)))
    remaining = list(range(len(supports)))
    while remaining:
        local = [t for t in remaining if all(pos[q] < nl for q in supports[t])]
        if local:
            steps.append(ShardStep("energy", items=local, pos=list(pos)))
            done = set(local)
            remaining = [t for t in remaining if t not in done]
            continue
        # the term that needs the fewest exchanges next; qubits that the remaining terms still flip stay local if possible
        t = min(remaining, key=lambda t: sum(pos[q] >= nl for q in supports[t]))
        wanted = {}
        for u in remaining:
            for q in supports[u]:
                wanted[q] = wanted.get(q, 0) + 1
        for q in [q for q in supports[t] if pos[q] >= nl]:
            cand = [v for v in range(n) if pos[v] < nl and v not in supports[t]]
            victim = min(cand, key=lambda v: (wanted.get(v, 0), v))
            steps.append(ShardStep("swap", rank_bit=pos[q] - nl, local_pos=pos[victim]))
            pos[q], pos[victim] = pos[victim], pos[q]
            swaps += 1
    return steps, swaps


class EngineShardBackend:
    """Local arithmetic on the GPU: one (n - g)-qubit handle of the engine; shards are torch complex128 CUDA tensors
    that the handle reads and writes in place (device-to-device on ONE stream, a torch stream of this object)."""

    def __init__(self, n_local: int, device):
        import torch
        from .engine import VQEEngine, Circuit
        self.torch, self.Circuit = torch, Circuit
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(device=self.device)
        self.engine = VQEEngine(n_local, self.device.index or 0)
        self.engine.set_stream(self.stream.cuda_stream)
        self.n_local = n_local

    def new_shard(self, values):
        t = self.torch.as_tensor(np.ascontiguousarray(values, np.complex128)).to(self.device)
        self.stream.wait_stream(self.torch.cuda.current_stream(self.device))
        t.record_stream(self.stream)      # allocated on the caller's stream, read and written on this object's from here on
        return t

    def exchange_context(self):
        """What AmplitudeShardedState._exchange runs under: this object's stream as torch's current one, so the
        half-shard swaps (their clones, the send / recv staging, the final copy_) sit in plain stream order with the
        handle's device-to-device copies - before them nothing had landed, after them nothing is read early."""
        return self.torch.cuda.stream(self.stream)

    def apply(self, shard, kind, q0, q1, pidx, theta):
        with self.torch.cuda.stream(self.stream):
            out = self.torch.empty_like(shard)      # (this stream's own block: torch's allocator reuses it in stream order)
            self.engine.set_init_state_dev(shard.data_ptr())
            self.engine.set_circuit(self.Circuit(kind, q0, q1, pidx, len(theta)))
            self.engine.get_state_dev(theta, out.data_ptr())
        shard.record_stream(self.stream)
        return out

    def energy(self, shard, xs, zs, cs):
        if not len(xs):
            return 0.0
        with self.torch.cuda.stream(self.stream):
            self.engine.set_init_state_dev(shard.data_ptr())
            self.engine.set_hamiltonian(xs, zs, cs)
            self.engine.set_circuit(self.Circuit.empty())
            e = self.engine.energy(np.zeros(0))
        shard.record_stream(self.stream)
        return e

    def halves(self, shard, local_pos):
        return shard.view(-1, 2, 1 << local_pos)

    def to_host(self, shard):
        self.stream.synchronize()
        return shard.cpu().numpy()

    def close(self):
        self.stream.synchronize()
        self.engine.set_stream(None)
        self.engine.close()


class AmplitudeShardedState:
    """Executor of a plan for the ranks this process holds: ``my_ranks`` = [rank] under torch.distributed (gloo in the
    CPU tests, RCCL on GPUs: the halves travel as send / recv pairs between the two partners), or all ranks of the
    world in ONE process (``my_ranks`` = range(world): the single-GPU emulation, exchange = device-to-device copy)."""

    def __init__(self, n, world, my_ranks, backend, group=None):
        self.n, self.world, self.g = n, world, _log2_exact(world)
        self.nl = n - self.g
        self.my_ranks = list(my_ranks)
        self.backend = backend
        self.group = group
        self.shards = {}
        self.exchanged_bytes = 0

    def load(self, psi0):
        """Initial state: this process keeps the slices [r 2^nl, (r+1) 2^nl) of its ranks (rank = top index bits)."""
        psi0 = np.asarray(psi0, np.complex128)
        for r in self.my_ranks:
            self.shards[r] = self.backend.new_shard(psi0[r << self.nl:(r + 1) << self.nl])

    def _exchange(self, k, local_pos):
        """One half-shard exchange, under the backend's ``exchange_context()`` if it has one: a backend that works on a
        stream of its own (EngineShardBackend) makes that stream the current one, so the exchange is ordered behind the
        copy that wrote the shard and ahead of the copy that reads it next.  A backend without the hook (host arrays)
        gets a null context."""
        ctx = getattr(self.backend, "exchange_context", None)
        with ctx() if ctx is not None else contextlib.nullcontext():
            self._exchange_in_order(k, local_pos)

    def _exchange_in_order(self, k, local_pos):
        bit = 1 << k
        done = set()
        for r in self.my_ranks:
            if r in done:
                continue
            p = r ^ bit
            b = (r >> k) & 1
            mine = self.backend.halves(self.shards[r], local_pos)[:, 1 - b, :]
            if p in self.shards:                                   # both partners live here: swap in place
                theirs = self.backend.halves(self.shards[p], local_pos)[:, b, :]
                tmp = mine.clone() if hasattr(mine, "clone") else mine.copy()
                mine[...] = theirs
                theirs[...] = tmp
                done.add(p)
                self.exchanged_bytes += int(np.prod(mine.shape)) * 16      # (the partner's half travels too)
            else:
                import torch
                import torch.distributed as dist
                t = mine if isinstance(mine, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mine))
                send = torch.view_as_real(t.contiguous()).clone()
                recv = torch.empty_like(send)
                if dist.get_backend(self.group) != "nccl" and send.is_cuda:
                    send = send.cpu()
                    recv = recv.cpu()
                ops = [dist.P2POp(dist.isend, send, p, self.group), dist.P2POp(dist.irecv, recv, p, self.group)]
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
                got = torch.view_as_complex(recv)
                if isinstance(mine, torch.Tensor):
                    mine.copy_(got.to(mine.device))
                else:
                    mine[...] = got.numpy()
            self.exchanged_bytes += int(np.prod(mine.shape)) * 16
            done.add(r)

    def run(self, steps, kind, q0, q1, pidx, theta, xmask, zmask, coeff):
        """Execute ``steps``; returns this process's part of <psi|H|psi> (the caller sums over processes)."""
        kind, q0, q1, pidx = (np.asarray(a) for a in (kind, q0, q1, pidx))
        theta = np.asarray(theta, np.float64)
        xmask, zmask = np.asarray(xmask, np.uint64), np.asarray(zmask, np.uint64)
        coeff = np.asarray(coeff)
        nl, e = self.nl, 0.0
        for st in steps:
            if st.kind == "swap":
                self._exchange(st.rank_bit, st.local_pos)
            elif st.kind == "gates":
                idx = np.asarray(st.items)
                pos = np.asarray(st.pos)
                k = kind[idx].astype(np.int32)
                a = pos[q0[idx]].astype(np.int32)
                two = (k == 0) | (k == 5)
                b = np.where(two, pos[np.where(two, q1[idx], 0)], -1).astype(np.int32)
                rot = (k >= 1) & (k <= 3)
                th = theta[pidx[idx][rot]]
                pl = np.where(rot, np.cumsum(rot) - 1, -1).astype(np.int32)
                for r in self.my_ranks:
                    self.shards[r] = self.backend.apply(self.shards[r], k, a, b, pl, th)
            else:                       # energy of the terms whose X support is local: Z factors on rank bits are signs
                pos = st.pos
                for r in self.my_ranks:
                    xs, zs, cs = [], [], []
                    for t in st.items:
                        x, z = int(xmask[t]), int(zmask[t])
                        xl = zl = 0
                        sign = 1.0
                        for q in range(self.n):
                            if (x >> q) & 1:
                                xl |= 1 << pos[q]
                            if (z >> q) & 1:
                                if pos[q] < nl:
                                    zl |= 1 << pos[q]
                                elif (r >> (pos[q] - nl)) & 1:
                                    sign = -sign
                        xs.append(xl), zs.append(zl), cs.append(coeff[t] * sign)
                    e += self.backend.energy(self.shards[r], np.array(xs, np.uint64), np.array(zs, np.uint64), np.array(cs))
        return e
