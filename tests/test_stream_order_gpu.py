"""GPU: stream order at the device-pointer seams.  The handle's own stream and every torch.cuda.Stream() are
non-blocking, so where the engine (vqe_set_init_state_dev, vqe_get_state_dev, vqe_batch_copy_energy) or the Python
layers on top (parallel.TermShardedEngine, EngineShardBackend, AmplitudeShardedState, the CUDA tensor target of the
resident fit) read or write a caller's device buffer asynchronously, stream order is all the ordering there is.  Every
test puts a fixed delay (tests/stream_order_helpers.py: a bounded spin of 30 ms, asserted to have lasted >= 10 ms) on
the producer's stream; a consumer that is not ordered behind the producer then reads a known decoy every time.  Each
seam test runs the negative control once: the same sequence with the consumer on a second stream and no wait must read
the decoy, else the delay opened no window and the test fails.  (That second stream is independent_stream()'s: one
that shares no hardware queue with the first, on which it would run in order by accident.)

Tolerances: energies 1e-10 and amplitudes 1e-12 against the oracle (those of test_engine_plumbing and
test_amp_shard_gpu), and bit for bit against the same calls made with full synchronisation.  The decoys are more than
1e-3 away (asserted on the CPU when a case is built)."""
import numpy as np
import pytest

import vqe_oracle as vo
from helpers import random_gates, random_hamiltonian, random_state
from stream_order_helpers import (MIN_DELAY_MS, DecoyPair, DelayedTorchBackend, control_reads_decoy, delay,
                                  delayed_engine_backend, heisenberg_case, independent_stream,
                                  logical_state)

pytestmark = pytest.mark.gpu
E_TOL, A_TOL = 1e-10, 1e-12
DEV = "cuda:0"

_CASES = {}


def _case(n):
    """The shapes of test_engine_plumbing: 25 Pauli terms, 4 circuits of 12 gates; a true and a decoy initial state,
    true and decoy thetas, and the oracle's energies / states of each combination a test needs.  Built once per n and
    never changed."""
    if n not in _CASES:
        rng, drng = np.random.default_rng(7000 + n), np.random.default_rng(9000 + n)
        ham = random_hamiltonian(n, 25, rng)
        raws = [random_gates(n, 12, rng) for _ in range(4)]
        psi0, psi0_decoy = random_state(n, rng), random_state(n, drng)
        th = [g[4] for g in raws]
        th_decoy = [drng.uniform(-np.pi, np.pi, t.size) for t in th]
        energy = lambda p0, g, t: vo.energy_pauli(vo.run_circuit(p0, *g[:4], t), *ham)
        e_batch = lambda p0, ths: np.array([energy(p0, g, t) for g, t in zip(raws, ths)])
        # circuit 0 at several thetas (vqe_energy_batch takes one circuit)
        th0 = np.array([th[0], th_decoy[0]] + [rng.uniform(-np.pi, np.pi, th[0].size) for _ in range(2)])
        e0 = lambda p0: np.array([energy(p0, raws[0], t) for t in th0])
        state0 = lambda p0: vo.run_circuit(p0, *raws[0][:4], th0[0])
        _CASES[n] = dict(
            n=n, ham=ham, raws=raws, th0=th0,
            init=DecoyPair(psi0, psi0_decoy, e0(psi0), e0(psi0_decoy)),
            state=DecoyPair(psi0, psi0_decoy, state0(psi0), psi0_decoy, every=False),
            thetas=DecoyPair(np.concatenate(th), np.concatenate(th_decoy), e_batch(psi0, th), e_batch(psi0, th_decoy)))
    return _CASES[n]


def _split(case, flat):
    out, off = [], 0
    for g in case["raws"]:
        out.append(np.asarray(flat[off:off + g[4].size]))
        off += g[4].size
    return out


def _engine(case, psi0=None):
    import tensorrl_qas_amd as tq
    eng = tq.VQEEngine(case["n"], 0)
    eng.set_init_state(case["init"].true if psi0 is None else psi0)
    eng.set_hamiltonian(*case["ham"])
    return eng


def _circuits(case):
    import tensorrl_qas_amd as tq
    return [tq.Circuit(*g[:4], g[4].size) for g in case["raws"]]


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).to(DEV)
    torch.cuda.synchronize()
    return t


def _bits(t):
    return t.cpu().numpy().tobytes()


# ---- sharded states under delay (AmplitudeShardedState and its backend) -----------------------------------------------
def _run_sharded(n, world, case, backend):
    import torch
    from tensorrl_qas_amd import parallel
    st = parallel.AmplitudeShardedState(n, world, range(world), backend)
    # the caller's stream: one that does not share a hardware queue with the backend's (on a shared queue an exchange
    # that is ordered with nothing would still run in order, by accident)
    with torch.cuda.stream(independent_stream(backend.stream)):
        st.load(case["psi0"])
        e = st.run(case["steps"], *case["gates"], *case["ham"])
        psi = logical_state([backend.to_host(st.shards[r]) for r in range(world)], case["steps"][-1].pos, n)
    ms = [d.ms for d in backend.delays]
    print(f"n {n} world {world}: {case['swaps']} swaps, {len(ms)} delays of {min(ms):.1f} .. {max(ms):.1f} ms, "
          f"|e - oracle| {abs(e - case['e']):.3e}, max |psi - oracle| {np.abs(psi - case['psi']).max():.3e}")
    assert case["swaps"] >= 1 and ms and min(ms) >= MIN_DELAY_MS
    return st, e, psi


@pytest.mark.parametrize("late", ["backend", "exchange"])
def test_sharded_state_with_a_late_torch_backend(late):
    """Both directions of the seam without the engine: "backend" - the copy that fills a new shard lands 30 ms late on
    the backend's stream, so an exchange that does not wait for that stream swaps zeros; "exchange" - the exchange is
    30 ms late on its stream, so a backend that does not wait for it reads the shard before the swap.
    Before the exchange ran under the backend's exchange_context() this test saw |e - oracle| = 1.5e-01 in both
    directions (max |psi - oracle| 1e-01); it prints the present figures."""
    n, world, G = 10, 4, 20
    case = heisenberg_case(n, world, G, 1004)
    backend = DelayedTorchBackend(n - 2, DEV, late=late)
    st, e, psi = _run_sharded(n, world, case, backend)
    assert abs(e - case["e"]) < E_TOL, (e, case["e"])
    assert np.abs(psi - case["psi"]).max() < A_TOL
    backend.close()


@pytest.mark.parametrize("n,world", [(14, 4), (16, 2)])       # 12-qubit handles (LDS-resident), 15-qubit handles (streaming)
def test_sharded_state_with_a_late_exchange_on_the_engine(n, world):
    """EngineShardBackend whose halves() delays the stream the exchange is about to use: the handle's next
    vqe_set_init_state_dev (an asynchronous copy on the backend's stream) must still copy the exchanged shard.
    (With the exchange on the caller's stream, as it was, |e - oracle| was 2.3e-02 and 2.6e-02 here.)"""
    import tensorrl_qas_amd as tq
    G = 16
    case = heisenberg_case(n, world, G, 100 * n + world)
    nl = n - (world.bit_length() - 1)
    backend = delayed_engine_backend(nl, DEV)
    st, e, psi = _run_sharded(n, world, case, backend)
    full = tq.VQEEngine(n)
    full.set_init_state(case["psi0"])
    full.set_hamiltonian(*case["ham"])
    full.set_circuit(tq.Circuit(*case["gates"][:4], case["gates"][4].size))
    e_full = full.energy(case["gates"][4])
    assert abs(e - e_full) < E_TOL and abs(e - case["e"]) < E_TOL, (e, e_full, case["e"])
    assert st.exchanged_bytes == case["swaps"] * world * (1 << nl) * 8
    assert np.abs(psi - case["psi"]).max() < A_TOL
    backend.close()
    full.close()


# ---- the engine's own device-pointer seams, on a caller-owned stream --------------------------------------------------
@pytest.mark.parametrize("n", [12, 14])
def test_set_init_state_dev_with_a_late_source(n):
    """vqe_set_init_state_dev copies asynchronously on the handle's stream: a source that the caller writes late on that
    stream is copied after the write."""
    import torch
    case = _case(n)
    true, decoy = _dev(case["init"].true), _dev(case["init"].decoy)
    eng = _engine(case, psi0=case["init"].decoy)
    eng.set_circuit(_circuits(case)[0])
    S = torch.cuda.Stream()
    eng.set_stream(S.cuda_stream)

    # full synchronisation
    src = decoy.clone()
    src.copy_(true)
    torch.cuda.synchronize()
    eng.set_init_state_dev(src.data_ptr())
    eng.sync()
    e_sync, psi_sync = eng.energy_batch(case["th0"]), eng.get_state(case["th0"][0])

    # the negative control: the source is written late on S, the handle copies on a second stream with no wait
    Q = independent_stream(S)
    src = decoy.clone()
    seen = {}
    eng.set_stream(Q.cuda_stream)          # (drains the stream it leaves: done here, before S is made late)

    def consume():
        eng.set_init_state_dev(src.data_ptr())
        seen["e"] = eng.energy_batch(case["th0"])

    ms = control_reads_decoy(lambda: src.copy_(true), consume,
                             lambda: np.abs(seen["e"] - case["init"].decoy_result).max() < E_TOL, S, Q)
    eng.set_stream(S.cuda_stream)

    # the test: delay, write, copy - all on S
    src = decoy.clone()
    torch.cuda.synchronize()
    d = delay(S)
    with torch.cuda.stream(S):
        src.copy_(true)
        eng.set_init_state_dev(src.data_ptr())
    e, psi = eng.energy_batch(case["th0"]), eng.get_state(case["th0"][0])
    print(f"n {n}: delay {d.ms:.1f} ms (control {ms:.1f} ms), max |e - oracle| {np.abs(e - case['init'].true_result).max():.3e}")
    assert d.ms >= MIN_DELAY_MS
    assert np.abs(e - case["init"].true_result).max() < E_TOL
    assert np.abs(psi - case["state"].true_result).max() < A_TOL
    assert np.array_equal(e, e_sync) and np.array_equal(psi, psi_sync)
    eng.set_stream(None)
    eng.close()


def _oracle_at(case, x):
    return np.array([vo.energy_pauli(vo.run_circuit(case["init"].true, *g[:4], t), *case["ham"])
                     for g, t in zip(case["raws"], _split(case, x))])


@pytest.mark.parametrize("n,mode", [(12, "energy"), (12, "minimize"), (12, "env_step"), (14, "energy"), (14, "reduction")])
def test_batch_copy_energy_behind_a_delayed_run(n, mode):
    """vqe_batch_copy_energy is a device-to-device copy on the handle's stream: behind a delayed run it copies that
    run's energies, and a clone enqueued behind it on the same stream reads them."""
    import torch
    case = _case(n)
    eng = _engine(case)
    S = torch.cuda.Stream()
    eng.set_stream(S.cuda_stream)
    eng.batch_load(_circuits(case), _split(case, case["thetas"].true))
    if mode == "env_step":
        eng.batch_set_new_gate([len(g[0]) - 1 for g in case["raws"]])
    if mode == "reduction":
        eng.batch_run_energy()          # the states the reduction sums over
        eng.sync()
    run = {"energy": eng.batch_run_energy, "reduction": eng.batch_run_reduction,
           "minimize": lambda: eng.batch_run_minimize(1.0, 1e-4, 30),
           "env_step": lambda: eng.batch_run_env_step(1.0, 1e-4, 30)}[mode]
    stale = case["thetas"].decoy_result          # what the buffer holds before: the energies of the decoy thetas

    # full synchronisation
    buf = _dev(stale)
    run()
    eng.sync()
    eng.batch_copy_energy(buf.data_ptr())
    eng.sync()
    out_sync = buf.clone()
    torch.cuda.synchronize()

    # the negative control: run and copy late on S, the clone on a second stream with no wait
    buf = _dev(stale)
    seen = {}

    def produce():
        run()
        eng.batch_copy_energy(buf.data_ptr())

    def consume():
        seen["out"] = buf.clone()

    ms = control_reads_decoy(produce, consume, lambda: _bits(seen["out"]) == stale.tobytes(), S)

    # the test: everything on S, synchronised only at the end
    buf = _dev(stale)
    d = delay(S)
    with torch.cuda.stream(S):
        run()
        eng.batch_copy_energy(buf.data_ptr())
        out = buf.clone()
    S.synchronize()
    x, f, _ = eng.batch_fetch()
    # an optimiser run: f is the energy at the x it returns; an energy run: at the thetas that were loaded
    ref = _oracle_at(case, x) if mode in ("minimize", "env_step") else case["thetas"].true_result
    print(f"n {n} {mode}: delay {d.ms:.1f} ms (control {ms:.1f} ms), max |f - oracle| {np.abs(f - ref).max():.3e}")
    assert d.ms >= MIN_DELAY_MS
    assert _bits(out) == f.tobytes() and _bits(out) == _bits(out_sync)
    assert np.abs(f - ref).max() < E_TOL
    eng.set_stream(None)
    eng.close()


@pytest.mark.parametrize("n", [12, 14])
def test_get_state_dev_into_a_buffer_the_stream_still_reads(n):
    """vqe_get_state_dev writes asynchronously on the handle's stream: a clone of the destination enqueued before the
    call still sees the old content (the engine did not write early), one enqueued after it sees the state."""
    import torch
    case = _case(n)
    eng = _engine(case)
    eng.set_circuit(_circuits(case)[0])
    S = torch.cuda.Stream()
    eng.set_stream(S.cuda_stream)
    theta, decoy = case["th0"][0], case["state"].decoy

    # full synchronisation
    dst = _dev(decoy)
    eng.get_state_dev(theta, dst.data_ptr())
    eng.sync()
    got_sync = dst.clone()
    torch.cuda.synchronize()

    # the negative control: S reads the destination late, the handle writes on a second stream with no wait - the late
    # reader finds the state where the decoy should still be.  (The other direction cannot be forced: the call waits
    # for the handle's stream on the host while it loads theta, and what it enqueues after that takes microseconds.)
    dst = _dev(decoy)
    seen = {}
    Q = independent_stream(S)
    eng.set_stream(Q.cuda_stream)

    def produce():
        seen["keep"] = dst.clone()

    ms = control_reads_decoy(produce, lambda: eng.get_state_dev(theta, dst.data_ptr()),
                             lambda: np.abs(seen["keep"].cpu().numpy() - case["state"].true_result).max() < A_TOL, S, Q)
    eng.set_stream(S.cuda_stream)

    # the test
    dst = _dev(decoy)
    d = delay(S)
    with torch.cuda.stream(S):
        keep = dst.clone()
        eng.get_state_dev(theta, dst.data_ptr())
        got = dst.clone()
    S.synchronize()
    err = np.abs(got.cpu().numpy() - case["state"].true_result).max()
    print(f"n {n}: delay {d.ms:.1f} ms (control {ms:.1f} ms), max |psi - oracle| {err:.3e}")
    assert d.ms >= MIN_DELAY_MS
    assert _bits(keep) == decoy.tobytes()
    assert err < A_TOL and _bits(got) == _bits(got_sync)
    eng.set_stream(None)
    eng.close()


@pytest.mark.parametrize("n", [12, 14])          # 12: the term-shard branch; 14: the amplitude-shard branch
def test_term_sharded_engine_energies_orders_the_callers_stream(n):
    """TermShardedEngine.energies at world 1 (no process group), the caller on a non-default stream C: the object's
    stream waits for C on the way in (whatever the caller still does with the previous result) and C waits for it on
    the way out (the caller reads the sum)."""
    import torch
    from tensorrl_qas_amd import parallel
    case = _case(n)
    eng = _engine(case)
    sh = parallel.TermShardedEngine(eng, 0, 1, DEV)
    assert eng.device_info()["lds_path"] == (n == 12)
    circs = _circuits(case)
    th, th2 = _split(case, case["thetas"].true), _split(case, case["thetas"].decoy)
    e1, e2 = case["thetas"].true_result, case["thetas"].decoy_result
    own = sh._stream
    C = independent_stream(own)          # (no hardware queue shared with the object's stream)

    def run_and_copy(buf):          # what energies() enqueues on the object's stream, without its two waits
        eng.batch_run_energy()
        eng.batch_copy_energy(buf.data_ptr())

    with torch.cuda.stream(C):
        # ---- way in: the caller still reads the first result on C when the second evaluation is asked for
        eng.batch_load(circs, th)
        r1 = sh.energies(4)
        first = r1.clone()
        C.synchronize()
        assert np.abs(first.cpu().numpy() - e1).max() < E_TOL
        eng.batch_load(circs, th2)
        seen = {}

        def produce():
            seen["keep"] = r1.clone()

        # the negative control: the same evaluation enqueued by hand on the object's stream with no wait for C
        ms_in = control_reads_decoy(produce, lambda: run_and_copy(r1),
                                    lambda: np.abs(seen["keep"].cpu().numpy() - e2).max() < E_TOL, C, own)
        eng.batch_load(circs, th)
        r1 = sh.energies(4)
        C.synchronize()
        eng.batch_load(circs, th2)
        d_in = delay(C)
        keep = r1.clone()
        r2 = sh.energies(4)
        second = r2.clone()
        C.synchronize()
        assert d_in.ms >= MIN_DELAY_MS
        assert _bits(keep) == _bits(first)
        assert np.abs(second.cpu().numpy() - e2).max() < E_TOL

        # ---- way out: the object's stream is late, a clone on C right after the call holds the right energies
        eng.batch_load(circs, th)
        assert r2.data_ptr() == sh._buf.data_ptr()          # (the buffer now holds the energies of the decoy thetas)
        stale = _bits(r2)
        seen = {}

        def consume():
            seen["c"] = sh._buf.clone()

        ms_out = control_reads_decoy(lambda: run_and_copy(sh._buf), consume, lambda: _bits(seen["c"]) == stale, own, C)
        assert _bits(sh._buf) == _bits(first)
        eng.batch_load(circs, th2)
        eng.batch_run_energy()
        eng.batch_copy_energy(sh._buf.data_ptr())          # the stale content again
        eng.sync()
        assert _bits(sh._buf) == stale
        eng.batch_load(circs, th)
        d_out = delay(own)
        c = sh.energies(4).clone()
        C.synchronize()
        assert d_out.ms >= MIN_DELAY_MS
        print(f"n {n}: delays {d_in.ms:.1f} / {d_out.ms:.1f} ms (controls {ms_in:.1f} / {ms_out:.1f} ms), "
              f"max |e - oracle| {np.abs(c.cpu().numpy() - e1).max():.3e}")
        assert _bits(c) == _bits(first)
    sh.close()
    eng.close()


def test_resident_fit_with_a_tensor_target_written_late():
    """The resident fit reads a CUDA tensor target on a stream of its own: StiefelAdam.minimize synchronises torch's
    current stream first, so a target that the caller writes late on that stream is the one the fit reads.  Every output
    has the bits of the same fit with a host target."""
    import torch
    import stiefel_oracle as so
    from mps2qc_resident_helpers import OPTIMISER
    from tensorrl_qas_amd import dmrg_to_qc as dq
    n, layers, batch, steps = 6, 2, 2, 5
    rng, drng = np.random.default_rng(606), np.random.default_rng(909)
    sites = so.brickwork_pairs(n, layers)
    G = len(sites)
    targets = lambda r: np.array([so.circuit_state(n, sites, so.random_unitaries(G, r)) for _ in range(batch)])
    init = np.array([so.random_unitaries(G, rng) for _ in range(batch)])

    def oracle_history(tg):
        out = []
        for b in range(batch):
            ref = so.StiefelAdam(*OPTIMISER)
            ref.init(init[b])
            out.append(ref.minimize(n, list(sites), tg[b], init[b], max_iter=steps, tol=1e-30, param_tol=0.0)[2])
        return np.array(out)

    tg, tg_decoy = targets(rng), targets(drng)
    pair = DecoyPair(tg, tg_decoy, oracle_history(tg), oracle_history(tg_decoy), every=False)

    def fit(target):
        opt = dq.StiefelAdam(*OPTIMISER, stream=True, update="device")
        opt.minimize(dq.BrickworkOverlap(n, np.array(sites, np.int32), target), init, max_iter=steps, tol=1e-30, param_tol=0.0)
        return dict(best_val=opt.best_val, opt_params=opt.opt_params, final_params=opt.final_params,
                    loss_history=np.array(opt.loss_history), n_iter=opt.n_iter, last_envs=opt.last_envs,
                    last_overlap=opt.last_overlap)

    host = fit(pair.true)
    assert np.abs(host["loss_history"] - pair.true_result).max() < 1e-10      # (test_resident_fit_matches_oracle's bound)
    true_dev = _dev(pair.true)
    C = torch.cuda.Stream()

    # the negative control: a reader on a second stream with no wait sees the decoy
    target = _dev(pair.decoy)
    seen = {}

    def consume():
        seen["t"] = target.clone()

    ms = control_reads_decoy(lambda: target.copy_(true_dev), consume, lambda: _bits(seen["t"]) == pair.decoy.tobytes(), C)

    target = _dev(pair.decoy)
    with torch.cuda.stream(C):
        d = delay(C)
        target.copy_(true_dev)
        late = fit(target)
    assert d.ms >= MIN_DELAY_MS
    print(f"delay {d.ms:.1f} ms (control {ms:.1f} ms), max |history - host target's| "
          f"{np.abs(late['loss_history'] - host['loss_history']).max():.3e}")
    for k in host:
        assert np.asarray(late[k]).tobytes() == np.asarray(host[k]).tobytes(), k
