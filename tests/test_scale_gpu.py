"""GPU: the kernels at the batch sizes the product runs them at, and device buffers beyond 4 GiB (tests/scale_cases.py).

A. Every entry point of the LDS-resident family with B = grid + 3 circuits, grid = CUs x workgroups per CU from
   device_info() after a one-circuit launch of the same kind: every CU is filled to its residency and a second round
   begins.  Copies of a circuit must agree bit for bit wherever they sit (slices indexed by the workgroup, the reuse of a
   persistent grid's slice, workgroups that start while others hold the CU's LDS); each distinct circuit at its last
   position must agree with the oracle.  Noisy streams are no copies of each other: every stream of the energy run is
   held to the oracle under its own draws, sixteen streams of the minimise run are trace-checked.
B. Launches whose state-sized buffers end past 4 GiB: the streaming path (n = 18, 1030 streams: energy, lock-step
   COBYLA, gradient, L-BFGS; n = 20, 260 streams: the shape of bench.py's heis20 object), 18 resident density matrices of
   the batched exact channel mode at n = 12 and the levels + 2 matrices of one circuit's gradient there, the COBYLA
   scratch of 6033 circuits of 202 parameters at n = 12, a Lanczos basis of 260 vectors at n = 20, psi and phi of 66 fits
   at n = 22 on both fit paths.  tests/test_scale_cases_cpu.py proves every crossing from the library's size rules.  The
   two fit paths ride along at n = 20.

Tolerances are the project's: 1e-10 on energies, 1e-10 x max(1, sum |c_k|) on gradients (and on the energies of the
gradient and L-BFGS launches, as their own tests have it), 1e-9 on trial points.  Every test prints B, grid, workgroups per
CU, the bytes the handle holds, the worst deviation from the oracle, the copy groups compared and the kernel time."""
import time

import numpy as np
import pytest

import lds_cases as lc
import scale_cases as sc
from helpers import shift_grad

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tq():
    import tensorrl_qas_amd as t
    return t


def _free():
    import torch
    return int(torch.cuda.mem_get_info()[0])


def _grid(eng):
    info = eng.device_info()
    return int(info["cu_count"]) * int(info["wg_per_cu"]), int(info["wg_per_cu"])


def _circs(tq, circuits):
    return [tq.Circuit(*g, th.size) for g, th in circuits]


def _at_occupancy(eng, K, run, seed, probe):
    """run(order): load the circuits of ``order`` and launch.  A one-circuit launch of circuit ``probe`` tells the grid;
    the batch of grid + 3 follows, and is laid out again should its own sizes have changed the residency.
    -> (order, grid, workgroups per CU)"""
    run(np.array([probe]))
    grid, wg = _grid(eng)
    for _ in range(3):
        order = sc.tile_order(K, grid, seed)
        run(order)
        now, wg = _grid(eng)
        if now == grid:
            assert order.size == grid + 3 and grid >= 1
            return order, grid, wg
        grid = now
    raise AssertionError("the grid did not settle")


def _report(label, B, grid, wg, free0, worst, groups, ms):
    print(f"{label}: B={B} grid={grid} wg_per_cu={wg} bytes held={free0 - _free()} worst deviation={worst:.2e} "
          f"copy groups={groups} kernel ms={ms:.2f}")


# ---- A. the LDS-resident family at occupancy ------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_energy_at_occupancy(tq, n):
    psi0, ham = lc.inputs(n)
    circuits = sc.energy_circuits(n)
    free0 = _free()
    eng = lc.engine(tq, n)
    cs = _circs(tq, circuits)

    def run(order):
        eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
        eng.batch_run_energy()

    order, grid, wg = _at_occupancy(eng, len(cs), run, n, probe=len(cs) - 1)
    _, f, _ = eng.batch_fetch(want_x=False)
    ms = eng.last_kernel_ms()
    groups = sc.assert_copies_identical(order, {"f": f})
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        ref = lc.oracle_energy(n, psi0, circuits[k][0], circuits[k][1], ham)
        worst = max(worst, sc.assert_close(f"energy n={n} circuit {k} at {p}", f[p], ref, lc.E_TOL))
    _report(f"energy n={n}", order.size, grid, wg, free0, worst, groups, ms)
    eng.close()


@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_minimize_at_occupancy(tq, n):
    psi0, ham = lc.inputs(n)
    circuits = sc.minimize_circuits(n)
    maxfun = sc.minimize_maxfun(n)
    sizes = [th.size for _, th in circuits]
    free0 = _free()
    eng = lc.engine(tq, n)
    cs = _circs(tq, circuits)

    def run(order):
        eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
        eng.batch_run_minimize(1.0, 1e-4, maxfun)

    order, grid, wg = _at_occupancy(eng, len(cs), run, n, probe=len(cs) - 1)
    x, f, nfev = eng.batch_fetch()
    xopt = eng.batch_fetch_xopt()
    ms = eng.last_kernel_ms()
    per = [sizes[k] for k in order]
    x, xopt = sc.split(x, per), sc.split(xopt, per)
    groups = sc.assert_copies_identical(order, {"x": x, "xopt": xopt, "f": f, "nfev": nfev})
    assert np.all((nfev >= 1) & (nfev <= maxfun))
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        assert np.array_equal(x[p], xopt[p])                   # no float32 rounding outside an environment step
        ref = lc.oracle_energy(n, psi0, circuits[k][0], x[p], ham)
        worst = max(worst, sc.assert_close(f"minimize n={n} circuit {k} at {p}", f[p], ref, lc.E_TOL))
    _report(f"minimize n={n} maxfun={maxfun}", order.size, grid, wg, free0, worst, groups, ms)
    eng.close()


@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_env_step_at_occupancy(tq, n):
    psi0, ham = lc.inputs(n)
    cases = sc.env_step_circuits(n)
    assert [c[2] >= 0 for c in cases] == [True, False, True, True]
    assert cases[0][0][0][cases[0][2]] != 0 and cases[2][0][0][cases[2][2]] == 0      # a new rotation, a new CNOT
    maxfun = sc.minimize_maxfun(n)
    sizes = [th.size for _, th, _ in cases]
    free0 = _free()
    eng = lc.engine(tq, n)
    cs = [tq.Circuit(*g, th.size) for g, th, _ in cases]

    def run(order):
        eng.batch_load([cs[k] for k in order], [cases[k][1] for k in order])
        eng.batch_set_new_gate([cases[k][2] for k in order])
        eng.batch_run_env_step(1.0, 1e-4, maxfun)

    order, grid, wg = _at_occupancy(eng, len(cs), run, n, probe=0)
    x, f, nfev = eng.batch_fetch()
    xopt = eng.batch_fetch_xopt()
    ms = eng.last_kernel_ms()
    per = [sizes[k] for k in order]
    x, xopt = sc.split(x, per), sc.split(xopt, per)
    groups = sc.assert_copies_identical(order, {"x": x, "xopt": xopt, "f": f, "nfev": nfev})
    assert np.all((nfev >= 1) & (nfev <= maxfun))
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        gates, th, ng = cases[k]
        _, _, hole = sc.pre_action(gates, th.size, ng)
        if hole >= 0:
            assert x[p][hole] == th[hole] == 0.0
        assert np.array_equal(x[p], xopt[p].astype(np.float32).astype(np.float64))
        ref = lc.oracle_energy(n, psi0, gates, x[p], ham)      # the FULL circuit at the rounded optimum
        worst = max(worst, sc.assert_close(f"env step n={n} circuit {k} at {p}", f[p], ref, lc.E_TOL))
    _report(f"env step n={n} maxfun={maxfun}", order.size, grid, wg, free0, worst, groups, ms)
    eng.close()


@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_energy_grad_at_occupancy(tq, n):
    """n = 13: the persistent grid with more circuits than workgroups; below, lambda lives in the LDS"""
    psi0, ham = lc.inputs(n)
    circuits = sc.grad_circuits(n)
    sizes = [th.size for _, th in circuits]
    scale = sc.grad_scale(ham)
    free0 = _free()
    eng = lc.engine(tq, n)
    cs = _circs(tq, circuits)

    def run(order):
        eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
        eng.batch_run_energy_grad()

    order, grid, wg = _at_occupancy(eng, len(cs), run, n, probe=len(cs) - 1)
    _, f, _ = eng.batch_fetch(want_x=False)
    g = sc.split(eng.batch_fetch_grad(), [sizes[k] for k in order])
    ms = eng.last_kernel_ms()
    groups = sc.assert_copies_identical(order, {"f": f, "grad": g})
    energy = lambda p0, k, a, b, p, t, h: lc.oracle_energy(n, p0, (k, a, b, p), t, h)
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        gates, th = circuits[k]
        g_ref = shift_grad(psi0, *gates, th, ham, energy)
        worst = max(worst, sc.assert_close(f"gradient n={n} circuit {k} at {p}", g[p], g_ref, 1e-10 * scale))
        sc.assert_close(f"gradient's energy n={n} circuit {k} at {p}", f[p], lc.oracle_energy(n, psi0, gates, th, ham), 1e-10 * scale)
    _report(f"energy_grad n={n}", order.size, grid, wg, free0, worst, groups, ms)
    eng.close()


@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_noisy_energy_at_occupancy(tq, n):
    """Every stream against the oracle under the draws of (seed, stream, evaluation 0)"""
    import c_oracle as co
    psi0, ham = lc.inputs(n)
    circuits = sc.noisy_energy_circuits(n)
    free0 = _free()
    eng = lc.engine(tq, n)
    cs = _circs(tq, circuits)

    def run(order):
        eng.set_noise(lc.P1, lc.P2, sc.NOISE_SEED)             # the evaluation counter starts at 0
        eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
        eng.batch_run_energy()

    order, grid, wg = _at_occupancy(eng, len(cs), run, n, probe=len(cs) - 1)
    _, f, _ = eng.batch_fetch(want_x=False)
    ms = eng.last_kernel_ms()
    ref, known, hit = np.empty(order.size), {}, 0
    for b, k in enumerate(order):
        gates, th = circuits[k]
        dr = co.noise_draws(sc.NOISE_SEED, b, 0, gates[0], lc.P1, lc.P2)
        hit += bool(np.any(dr))
        key = (int(k), dr.tobytes())
        if key not in known:
            known[key] = lc.oracle_energy(n, psi0, gates, th, ham, dr)
        ref[b] = known[key]
    assert hit > order.size // 2 and len(known) > order.size // 4      # most streams drew errors, and different ones
    worst = sc.assert_close(f"noisy energy n={n}, all {order.size} streams", f, ref, lc.E_TOL)
    _report(f"noisy energy n={n} ({len(known)} distinct trajectories)", order.size, grid, wg, free0, worst, 0, ms)
    eng.close()


@pytest.mark.parametrize("n", sc.LDS_SIZES)
def test_noisy_minimize_at_occupancy(tq, n):
    """The streams at the six pinned positions and ten more: every traced value against the oracle under the stream's
    draws, and the host COBYLA's walk (lc.check_trace).  The circuit of a traced stream is the first of its seeds whose
    walk under THAT stream's draws is decided."""
    import c_oracle as co
    maxfun = sc.noisy_maxfun(n)
    base = sc.noisy_energy_circuits(n)
    free0 = _free()
    eng = lc.engine(tq, n)
    noise = lambda b: (sc.NOISE_SEED, b, lc.P1, lc.P2)

    laid = {}

    def run(order):
        """the layout of a batch: the base circuit of each position, the traced positions' own decided circuits"""
        circuits = [base[k] for k in order]
        traced = sc.traced_positions(order.size - 3) if order.size > 1 else []
        for b in traced:
            circuits[b] = sc.noisy_circuit(n, sc.NOISY_TRACED_P[order[b] % 2], b, maxfun)
        laid["circuits"], laid["traced"] = circuits, traced
        eng.set_noise(lc.P1, lc.P2, sc.NOISE_SEED)
        eng.batch_set_trace(True)
        eng.batch_load([tq.Circuit(*g, th.size) for g, th in circuits], [th for _, th in circuits])
        eng.batch_run_minimize(1.0, 1e-4, maxfun)

    order, grid, wg = _at_occupancy(eng, len(base), run, n, probe=len(base) - 1)
    circuits, traced = laid["circuits"], laid["traced"]
    x, f, nfev = eng.batch_fetch()
    ms = eng.last_kernel_ms()
    assert np.all((nfev >= 1) & (nfev <= maxfun)) and np.all(np.isfinite(f)) and np.all(np.isfinite(x))
    assert len(traced) == 6 + sc.EXTRA_TRACED and set(sc.pinned_positions(grid)) <= set(traced)
    psi0, ham = lc.inputs(n)
    worst = 0.0
    for b in traced:
        g, th = circuits[b]
        ft, xt = eng.batch_fetch_trace(b, th.size)
        lc.check_trace(tq, n, g, th, ft, xt, int(nfev[b]), maxfun, noise(b))      # asserts lc.E_TOL and lc.X_TOL
        for k in range(int(nfev[b])):      # the figure check_trace asserts on, for the report
            dr = co.noise_draws(sc.NOISE_SEED, b, k + 1, g[0], lc.P1, lc.P2)
            worst = max(worst, abs(ft[k] - lc.oracle_energy(n, psi0, g, xt[k], ham, dr)))
    eng.batch_set_trace(False)
    _report(f"noisy minimize n={n} maxfun={maxfun}, {len(traced)} streams traced", order.size, grid, wg, free0, worst, 0, ms)
    eng.close()


@pytest.mark.parametrize("n", sc.WIDE_SIZES)
def test_wide_minimize_at_occupancy(tq, n):
    """The WIDE minimiser (a circuit above 64 parameters in the batch): the optimiser's arrays in the global scratch at
    scratch_begin[circuit], for grid + 3 circuits"""
    psi0, ham = lc.inputs(n)
    circuits = sc.wide_circuits(n)
    maxfun = sc.wide_maxfun()
    sizes = [th.size for _, th in circuits]
    free0 = _free()
    eng = lc.engine(tq, n)
    cs = _circs(tq, circuits)

    def run(order):
        eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
        eng.batch_run_minimize(1.0, 1e-4, maxfun)

    order, grid, wg = _at_occupancy(eng, len(cs), run, n, probe=0)
    x, f, nfev = eng.batch_fetch()
    ms = eng.last_kernel_ms()
    per = [sizes[k] for k in order]
    x = sc.split(x, per)
    groups = sc.assert_copies_identical(order, {"x": x, "f": f, "nfev": nfev})
    assert np.all((nfev >= 1) & (nfev <= maxfun))
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        q = eng.batch_cobyla_placement(p)
        assert (q["class"], q["pad"]) == sc.wide_class(n, sizes[k]), (n, k, p, q)
        ref = lc.oracle_energy(n, psi0, circuits[k][0], x[p], ham)
        worst = max(worst, sc.assert_close(f"wide minimize n={n} circuit {k} at {p}", f[p], ref, lc.E_TOL))
    _report(f"wide minimize n={n} maxfun={maxfun}", order.size, grid, wg, free0, worst, groups, ms)
    eng.close()


def test_more_circuits_than_a_grid_dimension_of_65535(tq):
    n, B = sc.MANY_N, sc.MANY_B
    psi0, ham = lc.inputs(n)
    circuits = sc.many_circuits()
    free0 = _free()
    eng = lc.engine(tq, n)
    cs = _circs(tq, circuits)
    order = sc.tile_order(len(cs), B - 3, 4)
    assert order.size == B > 65535
    eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
    eng.batch_run_energy()
    grid, wg = _grid(eng)
    _, f, _ = eng.batch_fetch(want_x=False)
    ms = eng.last_kernel_ms()
    groups = sc.assert_copies_identical(order, {"f": f})
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        ref = lc.oracle_energy(n, psi0, circuits[k][0], circuits[k][1], ham)
        worst = max(worst, sc.assert_close(f"energy n={n} circuit {k} at {p}", f[p], ref, lc.E_TOL))
    _report(f"energy n={n}, {B} workgroups", B, grid, wg, free0, worst, groups, ms)
    eng.close()


# ---- B. buffers beyond 4 GiB ----------------------------------------------------------------------------------------
def _stream_engine(tq, n, ham):
    eng = tq.VQEEngine(n, 0)
    eng.set_init_state(sc.stream_state(n))
    eng.set_hamiltonian(*ham)
    assert not eng.device_info()["lds_path"]
    return eng


def _stream_report(label, B, eng, free0, need, worst, groups, seconds):
    grid, wg = _grid(eng)
    held = free0 - _free()
    print(f"{label}: B={B} grid={grid} wg_per_cu={wg} (no LDS-resident launch: B is the y extent of the grids) bytes held={held} "
          f"(state-sized buffers {need}) worst deviation={worst:.2e} copy groups={groups} wall s={seconds:.2f}")


def _stream_energy(tq, case, n, B, lengths, which):
    need = sc.require_memory(case)
    ham = sc.stream_hamiltonian(n, which)
    circuits = sc.stream_circuits(n, lengths)
    order = sc.stream_order(len(circuits), B)
    free0 = _free()
    eng = _stream_engine(tq, n, ham)
    cs = _circs(tq, circuits)
    eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
    t0 = time.perf_counter()
    eng.batch_run_energy()
    _, f, _ = eng.batch_fetch(want_x=False)
    dt = time.perf_counter() - t0
    groups = sc.assert_copies_identical(order, {"f": f})
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        ref = sc.stream_oracle_energy(n, circuits[k][0], circuits[k][1], ham)
        worst = max(worst, sc.assert_close(f"{case} ({which}) circuit {k} at {p}", f[p], ref, lc.E_TOL))
    _stream_report(f"{case} n={n} {which}", B, eng, free0, need, worst, groups, dt)
    eng.close()


@pytest.mark.parametrize("which", ["heisenberg", "random"])
def test_stream_energy_past_4gib(tq, which):
    _stream_energy(tq, "stream_energy", sc.STREAM_N, sc.STREAM_B, sc.STREAM_LENGTHS, which)


def test_stream_energy_bench_shape_past_4gib(tq):
    """What bench.py's heis20 object runs with 256 streams, with 260"""
    _stream_energy(tq, "stream_energy_bench", sc.BENCH_N, sc.BENCH_B, sc.BENCH_LENGTHS, "heisenberg")


def test_stream_minimize_past_4gib(tq):
    """The lock-step device COBYLA: the same states over six evaluations"""
    case, n, B, maxfun = "stream_minimize", sc.STREAM_N, sc.STREAM_B, sc.STREAM_MAXFUN
    need = sc.require_memory(case)
    ham = sc.stream_hamiltonian(n, "heisenberg")
    circuits = [lc.cobyla_case(n, P, 65000 + P, maxfun=maxfun, ham=ham) for P in sc.STREAM_MIN_P]
    sizes = [th.size for _, th in circuits]
    order = sc.stream_order(len(circuits), B)
    free0 = _free()
    eng = _stream_engine(tq, n, ham)
    cs = _circs(tq, circuits)
    eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
    t0 = time.perf_counter()
    eng.batch_run_minimize(1.0, 1e-4, maxfun)
    x, f, nfev = eng.batch_fetch()
    dt = time.perf_counter() - t0
    x = sc.split(x, [sizes[k] for k in order])
    groups = sc.assert_copies_identical(order, {"x": x, "f": f, "nfev": nfev})
    assert np.all((nfev >= 1) & (nfev <= maxfun))
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        ref = sc.stream_oracle_energy(n, circuits[k][0], x[p], ham)
        worst = max(worst, sc.assert_close(f"{case} circuit {k} at {p}", f[p], ref, lc.E_TOL))
    _stream_report(f"{case} n={n} maxfun={maxfun}", B, eng, free0, need, worst, groups, dt)
    eng.close()


def test_stream_grad_past_4gib(tq):
    """psi and lambda, about 4 GiB each"""
    case, n, B = "stream_grad", sc.STREAM_N, sc.STREAM_B
    need = sc.require_memory(case)
    ham = sc.stream_hamiltonian(n, "heisenberg")
    scale = sc.grad_scale(ham)
    circuits = sc.stream_circuits(n, sc.STREAM_LENGTHS)
    sizes = [th.size for _, th in circuits]
    order = sc.stream_order(len(circuits), B)
    free0 = _free()
    eng = _stream_engine(tq, n, ham)
    eng.set_stream_grad()
    cs = _circs(tq, circuits)
    eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
    t0 = time.perf_counter()
    eng.batch_run_energy_grad()
    _, f, _ = eng.batch_fetch(want_x=False)
    g = sc.split(eng.batch_fetch_grad(), [sizes[k] for k in order])
    dt = time.perf_counter() - t0
    groups = sc.assert_copies_identical(order, {"f": f, "grad": g})
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        gates, th = circuits[k]
        worst = max(worst, sc.assert_close(f"{case} circuit {k} at {p}", g[p], sc.stream_shift_grad(n, gates, th, ham), 1e-10 * scale))
        sc.assert_close(f"{case} energy of circuit {k} at {p}", f[p], sc.stream_oracle_energy(n, gates, th, ham), 1e-10 * scale)
    _stream_report(f"{case} n={n}", B, eng, free0, need, worst, groups, dt)
    eng.close()


def test_stream_lbfgs_past_4gib(tq):
    """One iteration of the lock-step device L-BFGS on psi and lambda of 1030 streams"""
    case, n, B = "stream_lbfgs", sc.STREAM_N, sc.STREAM_B
    need = sc.require_memory(case)
    ham = sc.stream_hamiltonian(n, "heisenberg")
    scale = sc.grad_scale(ham)
    circuits = sc.stream_circuits(n, sc.STREAM_LENGTHS)
    sizes = [th.size for _, th in circuits]
    order = sc.stream_order(len(circuits), B)
    free0 = _free()
    eng = _stream_engine(tq, n, ham)
    eng.set_stream_lbfgs()
    cs = _circs(tq, circuits)
    eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
    maxfun = int(eng.lbfgs_opts(maxiter=1).maxfun)
    t0 = time.perf_counter()
    eng.batch_run_minimize_lbfgs(maxiter=1)
    x, f, nfev = eng.batch_fetch()
    nit, st = eng.batch_fetch_lbfgs_info()
    dt = time.perf_counter() - t0
    x = sc.split(x, [sizes[k] for k in order])
    groups = sc.assert_copies_identical(order, {"x": x, "f": f, "nfev": nfev, "nit": nit, "status": st})
    assert np.all((nfev >= 1) & (nfev <= maxfun)) and np.all((nit >= 0) & (nit <= 1))
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, len(cs))):
        gates, th = circuits[k]
        ref = sc.stream_oracle_energy(n, gates, x[p], ham)
        worst = max(worst, sc.assert_close(f"{case} circuit {k} at {p}", f[p], ref, 1e-10 * scale))
        assert f[p] <= sc.stream_oracle_energy(n, gates, th, ham) + 1e-10 * scale      # no step uphill
    _stream_report(f"{case} n={n} maxiter=1", B, eng, free0, need, worst, groups, dt)
    eng.close()


def test_dm_batched_past_4gib(tq):
    """Exact channel mode, 18 density matrices of 256 MiB resident in one chunk: energies, then four lock-step COBYLA
    evaluations (inside the initial simplex, whose points are fixed: no walk to decide), against the factorised oracle."""
    case, n, B = "dm_batched", sc.DM_N, sc.DM_B
    need = sc.require_memory(case)
    three, states, psi0, ham = sc.dm_problem()
    circuits = sc.dm_circuits()
    sizes = [c[4].size for c in circuits]
    assert len(set(sizes)) == 3 and len({len(c[0]) for c in circuits}) == 3
    order = sc.tile_order(len(circuits), B - 3, 12)
    free0 = _free()
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(*sc.DM_NOISE, 11)
    eng.set_noise_mode(1)
    eng.set_dm_batched(B)
    cs = [tq.Circuit(*c[:4], c[4].size) for c in circuits]
    eng.batch_load([cs[k] for k in order], [circuits[k][4] for k in order])
    t0 = time.perf_counter()
    eng.batch_run_energy()
    _, f, _ = eng.batch_fetch(want_x=False)
    dt = time.perf_counter() - t0
    info = eng.dm_batch_info()
    assert info["resident"] == B and info["chunks"] == 1, info      # nothing was chunked: slot 17 begins at 4.25 GiB
    groups = sc.assert_copies_identical(order, {"f": f})
    worst = 0.0
    last = sc.last_positions(order, len(cs))
    for k, p in enumerate(last):
        worst = max(worst, sc.assert_close(f"{case} energy of circuit {k} at {p}", f[p], sc.dm_oracle_energy(k, circuits[k][4]), lc.E_TOL))
    t0 = time.perf_counter()
    eng.batch_run_minimize(1.0, 1e-4, sc.DM_MAXFUN)
    x, fm, nfev = eng.batch_fetch()
    dt += time.perf_counter() - t0
    x = sc.split(x, [sizes[k] for k in order])
    groups += sc.assert_copies_identical(order, {"x": x, "f": fm, "nfev": nfev})
    assert np.all((nfev >= 1) & (nfev <= sc.DM_MAXFUN))
    for k, p in enumerate(last):
        worst = max(worst, sc.assert_close(f"{case} minimise, circuit {k} at {p}", fm[p], sc.dm_oracle_energy(k, x[p]), lc.E_TOL))
        assert fm[p] <= f[p]
    _stream_report(f"{case} n={n} levels={info['levels']} maxfun={sc.DM_MAXFUN}", B, eng, free0, need, worst, groups, dt)
    eng.close()


def test_lanczos_basis_past_4gib(tq):
    """260 basis vectors of 16 MiB and a budget of one pass through them (a tolerance no pass can meet): the checks of
    test_streaming_sizes - the reported residual is the host's through hamiltonian.apply, the vector has unit norm.
    Running out of budget is no error."""
    case, n, m = "lanczos", sc.LZ_N, sc.LZ_BASIS
    need = sc.require_memory(case)
    ham, _ = tq.hamiltonian.heisenberg(n)
    free0 = _free()
    eng = tq.VQEEngine(n, 0)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    t0 = time.perf_counter()
    val, vec, info = eng.lanczos("min", max_basis=m, max_matvec=m, tol=1e-300)
    dt = time.perf_counter() - t0
    host_r = float(np.linalg.norm(tq.hamiltonian.apply(ham, vec) - val * vec))
    print(f"{case}: theta={val:.12f} info={info} host residual={host_r:.6e} kernel ms={eng.last_kernel_ms():.1f}")
    # a basis smaller than asked for (the solver takes a quarter of the free memory at most) would restart before the budget
    assert info["status"] == 2 and info["matvecs"] == m and info["restarts"] == 0, info      # vector 259 was written and read
    worst = sc.assert_close(f"{case} residual", info["residual"], host_r, 1e-10)
    assert abs(np.linalg.norm(vec) - 1.0) <= 1e-12
    assert abs(float(np.vdot(vec, tq.hamiltonian.apply(ham, vec)).real) - val) <= 1e-10
    _stream_report(f"{case} n={n} max_basis={m}", m, eng, free0, need, worst, 0, dt)
    eng.close()


# ---- the offline fit above 16 qubits ----------------------------------------------------------------------------------
FIT_OPTIMISER = (3e-3, 0.9, 0.999, 1e-8)
_FIT = {}


def _fit_problem(n, batch):
    """One brickwork layer, a shared random target, ``batch`` starts, and the numpy restatement's two steps per start:
    made once, shared by the two paths."""
    import stiefel_oracle as so
    if (n, batch) not in _FIT:
        rng = np.random.default_rng(81000 + n)
        sites = so.brickwork_pairs(n, 1)
        G = len(sites)
        tg = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
        tg /= np.linalg.norm(tg)
        init = np.array([so.random_unitaries(G, rng) for _ in range(batch)])
        init.setflags(write=False)
        ref = []
        for b in range(batch):
            o = so.StiefelAdam(*FIT_OPTIMISER)
            o.init(init[b])
            ref.append(o.minimize(n, list(sites), tg, init[b], max_iter=2, tol=1e-30, param_tol=0.0))
        _FIT[(n, batch)] = (sites, tg, init, ref)
    return _FIT[(n, batch)]


def _fit_and_check(update, n, order, held, label):
    """The fits of ``order`` (which of the distinct starts each one begins from) on one path, FIT_STEPS = 2 steps: copies
    hold the same bits, each distinct start at its last position agrees with the oracle at the tolerances of
    tests/test_mps2qc_resident_gpu.py - histories and best_val 1e-10, gates 1e-9, unitarity 1e-12.  ``held``: the bytes of
    psi, phi and the partials by the library's size rules (the call frees them before it returns)."""
    from tensorrl_qas_amd import dmrg_to_qc as dq
    sites, tg, starts, ref = _fit_problem(n, int(max(order)) + 1)
    init = np.ascontiguousarray(starts[order])
    opt = dq.StiefelAdam(*FIT_OPTIMISER, stream=True, update=update)
    opt.init(init)
    t0 = time.perf_counter()
    opt.minimize(dq.BrickworkOverlap(n, np.array(sites, np.int32), tg), init, max_iter=2, tol=1e-30, param_tol=0.0)
    dt = time.perf_counter() - t0
    hist = [np.asarray(h, np.float64) for h in opt.loss_history]
    groups = sc.assert_copies_identical(order, {"history": hist, "final gates": list(opt.final_params), "best gates": list(opt.opt_params),
                                                "best_val": list(opt.best_val), "n_iter": list(opt.n_iter)})
    worst_h = worst_g = 0.0
    for k, p in enumerate(sc.last_positions(order, len(ref))):
        bv, bp, h, fin = ref[k]
        assert opt.n_iter[p] == len(h) == 2
        worst_h = max(worst_h, sc.assert_close(f"{label} history of start {k} at {p}", hist[p], h, 1e-10))
        sc.assert_close(f"{label} best_val of start {k} at {p}", opt.best_val[p], bv, 1e-10)
        worst_g = max(worst_g, sc.assert_close(f"{label} final gates of start {k} at {p}", opt.final_params[p], np.array(fin), 1e-9))
        sc.assert_close(f"{label} best gates of start {k} at {p}", opt.opt_params[p], np.array(bp), 1e-9)
        for g in opt.final_params[p]:
            assert np.max(np.abs(g @ g.conj().T - np.eye(4))) <= 1e-12
    print(f"{label}: B={len(order)} grid=0 wg_per_cu=0 (B is the y extent of the grids) bytes held={held} worst deviation: histories "
          f"{worst_h:.2e}, gates {worst_g:.2e} copy groups={groups} wall s={dt:.2f}")


@pytest.mark.parametrize("update", ["host", "device"], ids=["stream", "resident"])
def test_fit_at_twenty_qubits(update):
    """mps2qc_fit_brickwork_stream and _resident at n = 20 (the header promises 26 qubits; no other test goes above 16)"""
    _fit_and_check(update, 20, np.array([0, 1]), 2 * 2 * (16 << 20), f"fit n=20 {update}")


@pytest.mark.parametrize("update", ["host", "device"], ids=["stream", "resident"])
def test_fit_past_4gib(update):
    """n = 22, 66 fits from 2 distinct starts: psi and phi hold 66 x 64 MiB each"""
    case = "fit_stream" if update == "host" else "fit_resident"
    need = sc.require_memory(case)
    order = sc.stream_order(2, sc.FIT_B)
    _fit_and_check(update, sc.FIT_N, order, need, f"{case} n={sc.FIT_N}")


def test_trainable_scratch_past_4gib(tq):
    """The trainable regime (202 parameters at 12 qubits, the workgroup-wide context on the global scratch): so many
    circuits that the last one's optimiser arrays begin past 4 GiB of d_scratch.  B follows from the words the library
    reports for a circuit; maxfun = P + 1 + 4."""
    case, n, maxfun = "trainable_scratch", sc.TRAIN_N, sc.trainable_maxfun()
    need = sc.require_memory(case)
    psi0, ham = lc.inputs(n)
    circuits = sc.trainable_circuits()
    free0 = _free()
    eng = lc.engine(tq, n)
    cs = _circs(tq, circuits)
    eng.batch_load(cs, [th for _, th in circuits])
    q = eng.batch_cobyla_placement(0)
    assert (q["class"], q["pad"]) == ("block", 16) and q["words"] == sc.trainable_words(), q
    B = sc.trainable_batch(q["words"])
    assert (B - 1) * sc.scratch_stride(q["words"]) * 8 >= sc.LINE + 8 * q["words"]
    order = sc.stream_order(2, B)
    eng.batch_load([cs[k] for k in order], [circuits[k][1] for k in order])
    assert eng.batch_cobyla_placement(B - 1)["class"] == "block"
    eng.batch_run_minimize(1.0, 1e-4, maxfun)
    x, f, nfev = eng.batch_fetch()
    ms = eng.last_kernel_ms()
    grid, wg = _grid(eng)
    x = x.reshape(B, sc.TRAIN_P)
    groups = sc.assert_copies_identical(order, {"x": list(x), "f": f, "nfev": nfev})
    assert np.all((nfev >= 1) & (nfev <= maxfun))
    worst = 0.0
    for k, p in enumerate(sc.last_positions(order, 2)):
        ref = lc.oracle_energy(n, psi0, circuits[k][0], x[p], ham)
        worst = max(worst, sc.assert_close(f"{case} circuit {k} at {p}", f[p], ref, lc.E_TOL))
    _report(f"{case} n={n} P={sc.TRAIN_P} maxfun={maxfun} (scratch {need} bytes)", B, grid, wg, free0, worst, groups, ms)
    eng.close()


def test_dm_grad_stack_past_4gib(tq):
    """Exact channel gradient of ONE circuit of 15 .. 17 block levels and its twin: each keeps levels + 2 density matrices
    of 256 MiB, and the line runs through a circuit's own stack.  Against the factorised parameter shift, as
    tests/test_dm_large_gpu.py: E and the gradient to 1e-10 max(1, sum |c_k|)."""
    case, n = "dm_grad", sc.DM_N
    need = sc.require_memory(case)
    three, states, psi0, ham = sc.dm_problem()
    c = sc.dm_grad_circuit()
    levels = sc.dm_grad_levels()
    scale = sc.grad_scale(ham)
    free0 = _free()
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(*sc.DM_NOISE, 11)
    eng.set_noise_mode(1)
    eng.set_dm_batched(sc.DMG_R * (levels + 2))
    eng.set_dm_grad(1)
    circ = tq.Circuit(*c[:4], c[4].size)
    eng.batch_load([circ, circ], [c[4], c[4]])
    t0 = time.perf_counter()
    eng.batch_run_energy_grad()
    f = eng.batch_fetch(want_x=False)[1].copy()
    g = eng.batch_fetch_grad().reshape(2, -1)
    dt = time.perf_counter() - t0
    assert eng.dm_batch_info() == {"resident": sc.DMG_R, "chunks": 1, "evaluations": 1, "levels": levels}, eng.dm_batch_info()
    groups = sc.assert_copies_identical(np.array([0, 0]), {"f": f, "grad": list(g)})
    e_ref, g_ref = sc.dm_grad_oracle()
    worst = sc.assert_close(f"{case} gradient (twin)", g[1], g_ref, 1e-10 * scale)
    sc.assert_close(f"{case} energy (twin)", f[1], e_ref, 1e-10 * scale)
    assert np.abs(g_ref).max() > 1e-3
    _stream_report(f"{case} n={n} levels={levels}", 2, eng, free0, need, worst, groups, dt)
    eng.close()
