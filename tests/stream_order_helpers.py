"""Stream-order tests (tests/test_stream_order_gpu.py, the amp_sharded_gpu worker): a bounded delay on the producer's
stream, a decoy that a consumer which is not ordered behind the producer reads instead of the true value, the negative
control that shows the delay opens that window, and the test-only shard backends.

Why.  The handle's own stream and every ``torch.cuda.Stream()`` are non-blocking: nothing is ordered implicitly.  Where
the engine or the Python layers read or write a caller's device buffer asynchronously, a missing wait is silent as long
as producer and consumer are microseconds apart.  With ``delay`` between them the consumer reads a known stale value
every time.  The delay is a bounded spin (at most ``MAX_DELAY_MS``), never a loop, and every read is of a valid,
allocated tensor: a stale read by construction, not a fault.  Nothing here touches the GPU at import."""
import numpy as np

TARGET_DELAY_MS = 30.0       # per delay
MIN_DELAY_MS = 10.0          # what every test asserts of the delay it measured: three orders of magnitude above the
                             # microseconds between two enqueues; below it the calibration is broken and a test
                             # would pass vacuously
MAX_DELAY_MS = 100.0
DECOY_GAP = 1e-3
_CAL_CYCLES = 10 ** 7
_cycles_per_ms = None


def cycles_per_ms():
    """``torch.cuda._sleep`` cycles per millisecond on this device: one ``_sleep(10**7)`` timed with two events, once
    per process (after one untimed call that loads the kernel)."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(_CAL_CYCLES)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.0, ms
        _cycles_per_ms = _CAL_CYCLES / ms
        print(f"torch.cuda._sleep({_CAL_CYCLES}) took {ms:.3f} ms: {_cycles_per_ms:.0f} cycles per ms")
    return _cycles_per_ms


class Delay:
    """One enqueued spin; ``ms`` is what the two events around it measured (reading it waits for the spin's end, so
    read it after everything else has been enqueued)."""

    def __init__(self, start, end, asked_ms):
        self._start, self._end, self.asked_ms = start, end, asked_ms

    @property
    def ms(self):
        self._end.synchronize()
        return self._start.elapsed_time(self._end)


def delay(stream, ms=TARGET_DELAY_MS):
    """Enqueue a spin of ``ms`` milliseconds (capped at MAX_DELAY_MS) on ``stream``; returns the Delay that measures it.
    Tests assert ``.ms >= MIN_DELAY_MS``."""
    import torch
    ms = min(float(ms), MAX_DELAY_MS)
    cycles = int(ms * cycles_per_ms())
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record(stream)
        torch.cuda._sleep(cycles)
        end.record(stream)
    return Delay(start, end, ms)


class DecoyPair:
    """The true input of a case and a decoy of the same kind (a normalised state, a theta or an energy vector) drawn
    from another seed, with the oracle's result for each.  The results differ by more than DECOY_GAP - in every entry if
    ``every`` (energies), in the largest entry otherwise (amplitudes) - which is asserted here, on the CPU, when the case
    is built: a consumer that read the decoy cannot pass a 1e-10 comparison with the true result."""

    def __init__(self, true, decoy, true_result, decoy_result, every=True):
        self.true, self.decoy = np.ascontiguousarray(true), np.ascontiguousarray(decoy)
        self.true_result, self.decoy_result = np.asarray(true_result), np.asarray(decoy_result)
        assert self.true.shape == self.decoy.shape and self.true.dtype == self.decoy.dtype
        d = np.abs(self.true_result - self.decoy_result)
        self.gap = float(d.min() if every else d.max())
        assert self.gap > DECOY_GAP, self.gap
        for a in (self.true, self.decoy, self.true_result, self.decoy_result):
            a.setflags(write=False)


def independent_stream(of, tries=8, probe_ms=2.0):
    """A fresh torch stream whose work runs WHILE ``of`` is busy.  Needed because the runtime multiplexes streams onto a
    few hardware queues (4 by default): two streams that happen to share one run in order by accident, which hides a
    missing wait and would make a negative control fail for no reason of the code's.  Bounded: at most ``tries``
    candidates (torch hands its pool's streams out round-robin), one spin of ``probe_ms`` each; a candidate is taken
    when a kernel on it has finished while ``of`` still spins."""
    import torch
    torch.cuda.synchronize(of.device)
    x = torch.zeros(8, device=of.device)
    torch.cuda.synchronize(of.device)
    for _ in range(tries):
        q = torch.cuda.Stream(device=of.device)
        if q.cuda_stream == of.cuda_stream:
            continue
        d = delay(of, probe_ms)
        with torch.cuda.stream(q):
            x.add_(1)
        q.synchronize()
        free = not d._end.query()
        of.synchronize()
        if free:
            return q
    raise AssertionError(f"none of {tries} streams ran concurrently with the given one")


def control_reads_decoy(produce, consume, stale, producer_stream=None, consumer_stream=None, ms=TARGET_DELAY_MS):
    """The negative control of a seam test: the same sequence with the consumer placed by the test itself on a second
    non-blocking stream and NO wait.  ``produce()`` runs with the producer's stream current, behind a delay;
    ``consume()`` right after it with the consumer's stream current (``independent_stream`` of the producer's unless
    the test names one it chose that way); ``stale()`` is evaluated once both streams have drained and must be true:
    the consumer observed the decoy / stale value, i.e. the delay really opens the window on this machine.  If not, the
    test fails (it does not skip).  Returns the measured delay in ms (>= MIN_DELAY_MS, asserted).  Every tensor read
    here is valid and allocated."""
    import torch
    P = producer_stream if producer_stream is not None else torch.cuda.Stream()
    Q = consumer_stream if consumer_stream is not None else independent_stream(P)
    assert P.cuda_stream != Q.cuda_stream and P.cuda_stream != 0 and Q.cuda_stream != 0
    torch.cuda.synchronize()
    d = delay(P, ms)
    with torch.cuda.stream(P):
        produce()
    with torch.cuda.stream(Q):
        consume()
    Q.synchronize()
    window = not d._end.query()          # the consumer had drained while the producer's delay was still spinning
    P.synchronize()
    assert d.ms >= MIN_DELAY_MS, d.ms
    assert stale(), f"the unordered consumer did not observe the stale value (consumer done inside the delay: {window})"
    return d.ms


# ---- shard backends of the tests ---------------------------------------------------------------------------------------
class DelayedTorchBackend:
    """Test-only backend of parallel.AmplitudeShardedState: shards are CUDA tensors, the arithmetic is the C oracle's on
    the host, and everything this object does to a shard happens late on a non-blocking stream of its own - as the
    engine's device-to-device copies do, but 30 ms late instead of microseconds.  ``apply`` hands out a zeroed tensor
    that the new shard reaches only behind a delay, and ``apply`` and ``energy`` read a shard on the backend's stream.
    ``late`` says which side of the seam is late: "backend" - the copy into the new shard and the read of ``energy`` sit
    behind a delay on the backend's stream, so an exchange that is not ordered behind that stream swaps zeros;
    "exchange" - ``halves`` delays the stream the exchange is about to use, so a backend that is not ordered behind the
    exchange reads the shard before the swap.  (Both at once would hide the first: the exchange's delay would outlast
    the copy's.)  Offers the hook of EngineShardBackend."""

    def __init__(self, n_local, device="cuda:0", late="backend"):
        import torch
        assert late in ("backend", "exchange")
        self.late = late
        self.torch, self.n_local = torch, n_local
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(device=self.device)
        self.delays = []

    def _delay(self, stream):
        self.delays.append(delay(stream))

    def new_shard(self, values):
        t = self.torch.as_tensor(np.ascontiguousarray(values, np.complex128)).to(self.device)
        self.stream.wait_stream(self.torch.cuda.current_stream(self.device))
        t.record_stream(self.stream)
        return t

    def exchange_context(self):
        return self.torch.cuda.stream(self.stream)

    def _read(self, shard):
        with self.torch.cuda.stream(self.stream):
            return shard.cpu().numpy()          # (synchronises the backend's stream, and no other)

    def apply(self, shard, kind, q0, q1, pidx, theta):
        import c_oracle as co
        new = co.run_circuit(self.n_local, self._read(shard), kind, q0, q1, pidx, theta)
        cur = self.torch.cuda.current_stream(self.device)
        staging = self.torch.from_numpy(new).to(self.device)
        out = self.torch.zeros_like(staging)
        cur.synchronize()                       # staging and the zeros are there
        if self.late == "backend":
            self._delay(self.stream)
        with self.torch.cuda.stream(self.stream):
            out.copy_(staging)
        staging.record_stream(self.stream)
        out.record_stream(self.stream)
        return out

    def energy(self, shard, xs, zs, cs):
        if not len(xs):
            return 0.0
        import c_oracle as co
        if self.late == "backend":
            self._delay(self.stream)
        return co.energy_pauli(self.n_local, self._read(shard), xs, zs, cs)

    def halves(self, shard, local_pos):
        if self.late == "exchange":
            self._delay(self.torch.cuda.current_stream(self.device))
        return shard.view(-1, 2, 1 << local_pos)

    def to_host(self, shard):
        self.stream.synchronize()
        return shard.cpu().numpy()

    def close(self):
        self.stream.synchronize()


def delayed_engine_backend(n_local, device="cuda:0"):
    """parallel.EngineShardBackend whose ``halves()`` enqueues a delay on the stream the exchange is about to use
    (torch's current one) before it returns the view, and whose view delays its ``copy_`` once more: the next ``apply`` /
    ``energy`` of the handle copies a shard that an unordered exchange has not written yet.  ``.delays``: the Delay
    objects, for the >= MIN_DELAY_MS assertion."""
    from tensorrl_qas_amd import parallel

    import torch
    delays = []

    class LateCopy(torch.Tensor):
        """The view that halves() hands out: its copy_ - the last thing a cross-process exchange does to the shard,
        after the host hop has drained the stream - sits behind a delay of its own."""

        def copy_(self, src, non_blocking=False):
            delays.append(delay(torch.cuda.current_stream(self.device)))
            return super().copy_(src, non_blocking)

    class DelayedEngineShardBackend(parallel.EngineShardBackend):
        def __init__(self, n_local, device):
            super().__init__(n_local, device)
            self.delays = delays

        def halves(self, shard, local_pos):
            delays.append(delay(self.torch.cuda.current_stream(self.device)))
            return super().halves(shard, local_pos).as_subclass(LateCopy)

    return DelayedEngineShardBackend(n_local, device)


def logical_state(shards_host, pos, n):
    """The shards of a plan's last step, concatenated in rank order, put back in logical order (``pos``: the
    positions of the last step) - the reassembly of tests/test_amp_shard_gpu.py."""
    phys = np.concatenate(shards_host)
    idx = np.arange(1 << n)
    src = np.zeros_like(idx)
    for q in range(n):
        src |= ((idx >> q) & 1) << pos[q]          # logical index -> physical index
    return phys[src]


def heisenberg_case(n, world, G, seed):
    """psi0, Heisenberg chain, random gates, the plan and the oracle's state and energy of one sharded-state case."""
    import tensorrl_qas_amd as tq
    import vqe_oracle as vo
    from tensorrl_qas_amd import parallel
    from helpers import random_gates, random_state
    rng = np.random.default_rng(seed)
    psi0 = random_state(n, rng)
    hh, _ = tq.hamiltonian.heisenberg(n)
    ham = (hh.xmask, hh.zmask, hh.coeff)
    gates = random_gates(n, G, rng)
    steps, swaps = parallel.plan_amplitude_sharding(n, world, *gates[:3], ham[0])
    psi = vo.run_circuit(psi0, *gates)
    return dict(psi0=psi0, ham=ham, gates=gates, steps=steps, swaps=swaps, psi=psi, e=vo.energy_pauli(psi, *ham))
