"""GPU: the case table of tests/stream_cases.py - circuits and Hamiltonians built to reach every branch of the streaming
path's device planners (k_t_plan_ops, k_t_plan_energy; certified on the CPU by tests/test_tile_plan_cpu.py) - through
the C ABI against the oracle.  Tolerances are the project's: amplitudes 1e-12, energies 1e-10, gradients
1e-10 max(1, sum |c|) against the exact parameter shift.  Every test prints its worst errors.  n = 14 or 16 only."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import stream_cases as sc
import su4_helpers as s4
import tile_plan_model as tm
import vqe_oracle as vo

pytestmark = pytest.mark.gpu

E_TOL = 1e-10
A_TOL = 1e-12
CIRCUITS = sc.circuit_cases()
HAMS = sc.hamiltonian_cases()
GROUPS = ("flip", "chunk", "low", "pass", "degenerate", "su4")


def _psi0(n, _cache={}):
    if n not in _cache:
        rng = np.random.default_rng(1400 + n)
        v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
        _cache[n] = v / np.linalg.norm(v)
    return _cache[n]


def _thetas(name, P):
    """The nominal angles of a case and two perturbed vectors."""
    rng = np.random.default_rng(zlib.crc32(("theta:" + name).encode()))
    th = rng.uniform(-np.pi, np.pi, P)
    return th, th[None, :] + rng.normal(size=(2, P))


def _circuit(gates):
    import tensorrl_qas_amd as tq
    if not gates:
        return tq.Circuit.empty()
    kind, q0, q1, pidx, P = sc.gate_arrays(gates)
    return tq.Circuit(kind, q0, q1, pidx, P)


def _state(n, gates, th):
    if not gates:
        return _psi0(n)
    kind, q0, q1, pidx, _ = sc.gate_arrays(gates)
    return s4.run_circuit(_psi0(n), kind, q0, q1, pidx, th)


def _energy_of(psi, ham):
    return vo.energy_pauli(psi, *ham) if len(ham[0]) else 0.0


def _engine(n, stream_grad=False):
    import tensorrl_qas_amd as tq
    eng = tq.VQEEngine(n, 0)
    eng.set_init_state(_psi0(n))
    assert not eng.device_info()["lds_path"]
    if stream_grad:
        eng.set_stream_grad()
    return eng


@pytest.fixture
def engine():
    """_engine, closed when the test ends - whether it passed or not."""
    made = []

    def make(n, stream_grad=False):
        made.append(_engine(n, stream_grad))
        return made[-1]
    yield make
    for eng in made:
        eng.close()


def _run_circuit_case(eng, name, n, gates, ham):
    """-> (worst amplitude error, worst energy error) of one case: energy on a fresh plan, the state on the cached
    circuit plan, two perturbed angle vectors as a batch."""
    P = sc.gate_arrays(gates)[4] if gates else 0
    th, ths = _thetas(name, P)
    eng.set_hamiltonian(*ham)
    eng.set_circuit(_circuit(gates))
    psi = _state(n, gates, th)
    de = abs(eng.energy(th) - _energy_of(psi, ham))
    da = float(np.abs(eng.get_state(th) - psi).max())
    if P:
        got = eng.energy_batch(ths)
        for i in range(2):
            de = max(de, abs(got[i] - _energy_of(_state(n, gates, ths[i]), ham)))
    return da, de


@pytest.mark.parametrize("group", GROUPS)
def test_circuit_cases(group, engine):
    engines, worst = {}, {}
    for name, grp, n, gates, ham in CIRCUITS:
        if grp != group:
            continue
        if n not in engines:
            engines[n] = engine(n)
        worst[name] = _run_circuit_case(engines[n], name, n, gates, ham)
    assert worst
    wa, we = max(v[0] for v in worst.values()), max(v[1] for v in worst.values())
    print("circuit cases [%s]: %d cases, worst amplitude error %.2e, worst energy error %.2e" % (group, len(worst), wa, we))
    bad = {k: v for k, v in worst.items() if not (v[0] < A_TOL and v[1] < E_TOL)}
    assert not bad, bad


def test_hamiltonian_cases(engine):
    """Every Hamiltonian case behind the empty circuit and behind the two-pass circuit (the 217 / 218 group pair behind
    the empty one only): 217 X-mask groups still run on the tiled kernels, 218 switch the same handle to the untiled
    ones, and back."""
    n = sc.N
    eng = engine(n)
    worst = {}
    for bg in ("empty", "two_pass"):
        gates = sc.background(bg, n)
        P = sc.gate_arrays(gates)[4] if gates else 0
        th, ths = _thetas("background:" + bg, P)
        states = [_state(n, gates, th)] + [_state(n, gates, t) for t in (ths if P else [])]
        circ = _circuit(gates)
        for name, hn, ham, backgrounds in HAMS:
            if bg not in backgrounds:
                continue
            assert hn == n
            eng.set_hamiltonian(*ham)
            eng.set_circuit(circ)
            got = [eng.energy(th)] + (list(eng.energy_batch(ths)) if P else [])
            worst["%s/%s" % (name, bg)] = max(abs(g - _energy_of(psi, ham)) for g, psi in zip(got, states))
            if not len(ham[0]):
                assert got[0] == 0.0
    print("hamiltonian cases: %d runs, worst energy error %.2e (%s)" % (len(worst), max(worst.values()), max(worst, key=worst.get)))
    bad = {k: v for k, v in worst.items() if not v < E_TOL}
    assert not bad, bad
    assert "ham_217_groups/empty" in worst and "ham_218_groups/empty" in worst and "ham_empty/two_pass" in worst


@pytest.mark.parametrize("prefix", [0, 1, 2])
def test_gradient(prefix, engine):
    """The streaming adjoint gradient on the flip-group circuits and on a three-pass circuit, each behind 0, 1 and 2
    extra RZ.  The backward kernel sweeps aligned groups of three ops from op 0; what that reaches is certified by
    tests/test_tile_plan_cpu.py::test_sweep_kernels_reach_their_generic_flip_codes: at every prefix one triple of each
    sweep3_* circuit is an aligned group, so the XOR-of-two-slots exchange (flip code 3) runs with RX, RY and RYY at
    each of the three alignments; in the other circuits the dependent op mostly meets its slots in the forward pass's
    chunks only, whose boundaries the prefix moves as well."""
    n = sc.N
    eng = engine(n, stream_grad=True)
    psi0 = _psi0(n)
    worst_e = worst_g = 0.0
    bad = {}
    cases = [c for c in CIRCUITS if c[1] == "flip" or c[0] == "pass_three"]
    assert len(cases) == 27
    for name, _, cn, gates, ham in cases:
        assert cn == n
        gates = [(sc.RZ, q, -1) for q in (sc.A, 2)[:prefix]] + gates
        kind, q0, q1, pidx, P = sc.gate_arrays(gates)
        th = _thetas("grad:%s:%d" % (name, prefix), P)[0]
        eng.set_hamiltonian(*ham)
        eng.set_circuit(_circuit(gates))
        e, g = eng.energy_grad(th)
        scale = max(1.0, float(np.abs(ham[2]).sum()))
        de = abs(e - s4.energy(psi0, kind, q0, q1, pidx, th, ham)) / scale
        dg = float(np.abs(g - s4.shift_grad(psi0, kind, q0, q1, pidx, th, ham)).max()) / scale
        worst_e, worst_g = max(worst_e, de), max(worst_g, dg)
        if not (de <= 1e-10 and dg <= 1e-10):
            bad[name] = (de, dg)
    print("gradient cases [prefix %d]: %d circuits, worst energy error %.2e, worst gradient error %.2e (both / max(1, sum |c|))"
          % (prefix, len(cases), worst_e, worst_g))
    assert not bad, bad


def test_mixed_batch(engine):
    """One resident batch of streams with one, two and three circuit passes, an empty circuit and a flip-code circuit:
    k_t_ops skips the streams whose passes are over and hands each stream's last pass to the fused instantiation.
    Every stream equals its single run bit for bit and the oracle to 1e-10, in both stream orders."""
    n = sc.N
    by_name = {c[0]: c for c in CIRCUITS}
    names = ["pass_full_basis", "pass_two", "pass_three", "empty_circuit", "flip_ry_7"]
    ham = sc.H12()
    assert [tm.summarize(n, by_name[k][3], ham)["passes"] for k in names] == [1, 2, 3, 1, 1]
    gates = [by_name[k][3] for k in names]
    thetas = [_thetas("batch:" + k, sc.gate_arrays(g)[4] if g else 0)[0] for k, g in zip(names, gates)]
    refs = [_energy_of(_state(n, g, t), ham) for g, t in zip(gates, thetas)]
    eng = engine(n)
    eng.set_hamiltonian(*ham)
    single = []
    for g, t in zip(gates, thetas):
        eng.set_circuit(_circuit(g))
        single.append(eng.energy(t))
    worst = 0.0
    for order in (list(range(len(names))), list(range(len(names)))[::-1]):
        eng.batch_load([_circuit(gates[i]) for i in order], [thetas[i] for i in order])
        eng.batch_run_energy()
        f = eng.batch_fetch(want_x=False)[1]
        for k, i in enumerate(order):
            assert f[k] == single[i], (names[i], f[k], single[i])
            worst = max(worst, abs(f[k] - refs[i]))
    print("mixed batch: worst energy error %.2e" % worst)
    assert worst < E_TOL


def _moved(gates, n, shift):
    """The same gate list on other qubits."""
    return [(k, (a + shift) % n, (b + shift) % n if b >= 0 else -1) for k, a, b in gates]


def test_plan_cache(engine):
    """One handle through everything that must invalidate (or may keep) the cached plans of stream_evaluate."""
    import tensorrl_qas_amd as tq
    n = sc.N
    gA = sc.two_pass_circuit(n)
    gB = _moved(gA, n, 5)
    kA, kB = sc.gate_arrays(gA), sc.gate_arrays(gB)
    assert kA[0].tolist() == kB[0].tolist() and kA[4] == kB[4] and kA[1].tolist() != kB[1].tolist()
    ham1, ham2 = sc.H12(), sc.random_complex_hamiltonian(n, 12, "plan_cache")
    assert len(set(ham1[0].tolist())) == len(set(ham2[0].tolist())) and ham1[0].tolist() != ham2[0].tolist()
    assert tm.summarize(n, gB, ham2)["fused_groups"] > 0          # the amplitude shards below: a fused pass that holds groups
    th = _thetas("plan_cache", kA[4])[0]
    psiA, psiB = _state(n, gA, th), _state(n, gB, th)
    eng = engine(n)
    errs = {}
    eng.set_hamiltonian(*ham1)
    eng.set_circuit(_circuit(gA))
    errs["A"] = abs(eng.energy(th) - _energy_of(psiA, ham1))
    eng.set_circuit(_circuit(gB))
    errs["B"] = abs(eng.energy(th) - _energy_of(psiB, ham1))
    assert np.abs(eng.get_state(th) - psiB).max() < A_TOL          # a circuit-only plan ...
    errs["B after get_state"] = abs(eng.energy(th) - _energy_of(psiB, ham1))      # ... then the energy again
    eng.set_hamiltonian(*ham2)
    full = _energy_of(psiB, ham2)
    errs["new hamiltonian"] = abs(eng.energy(th) - full)
    parts = []
    for r in (1, 0):
        eng.set_term_shard(r, 2)
        parts.append(eng.energy(th))
    errs["term shards"] = abs(sum(parts) - full)
    eng.set_term_shard(0, 1)
    with pytest.raises(tq.VQEError):
        eng.set_amplitude_shard(0, 16)                              # 8 tiles at n = 14
    parts = []
    for r in range(8):                                              # one tile per rank
        eng.set_amplitude_shard(r, 8)
        parts.append(eng.energy(th))
    errs["amplitude shards"] = abs(sum(parts) - full)
    eng.set_amplitude_shard(0, 1)
    errs["unsharded again"] = abs(eng.energy(th) - full)
    th2 = _thetas("plan_cache:2", kA[4])[0]
    for tag, g in (("batch 1", gA), ("batch 2", gB)):               # equal shapes, different circuits
        eng.batch_load([_circuit(g), _circuit(g)], [th, th2])
        eng.batch_run_energy()
        f = eng.batch_fetch(want_x=False)[1]
        errs[tag] = max(abs(f[0] - _energy_of(_state(n, g, th), ham2)), abs(f[1] - _energy_of(_state(n, g, th2), ham2)))
    print("plan cache: " + ", ".join("%s %.1e" % kv for kv in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < E_TOL}
    assert not bad, bad


# ---- the kernels behind the two switches, each in a process of its own (the switches are read once per process) -------
def child_main():
    """Flip-code, chunk-limit and pass-limit circuits and the half-group Hamiltonians under whatever switches the
    environment sets; one JSON line of worst errors."""
    worst = {"amplitude": 0.0, "energy": 0.0, "cases": 0}
    engines = {}
    for name, grp, n, gates, ham in CIRCUITS:
        if grp not in ("flip", "chunk", "pass"):
            continue
        if n not in engines:
            engines[n] = _engine(n)
        da, de = _run_circuit_case(engines[n], name, n, gates, ham)
        worst["amplitude"], worst["energy"], worst["cases"] = max(worst["amplitude"], da), max(worst["energy"], de), worst["cases"] + 1
    n = sc.N
    for bg in ("empty", "two_pass"):
        gates = sc.background(bg, n)
        for name, _, ham, backgrounds in HAMS:
            if name.startswith("ham_half") and bg in backgrounds:
                _, de = _run_circuit_case(engines[n], "child:" + bg, n, gates, ham)
                worst["energy"], worst["cases"] = max(worst["energy"], de), worst["cases"] + 1
    print(json.dumps(worst))


@pytest.mark.parametrize("switch", ["VQE_STREAM_TILED", "VQE_STREAM_FUSE"])
def test_other_kernels(switch, tmp_path):
    """VQE_STREAM_TILED=0: the one-sweep-per-four-ops kernels (k_s_opk<4>; flip_xor3_aligned4 is the op whose mask is the
    XOR of the three before it in an aligned group of four; the generic flip codes 3 and 7 of that kernel are certified
    for these circuits by tests/test_tile_plan_cpu.py::test_sweep_kernels_reach_their_generic_flip_codes).  VQE_STREAM_FUSE=0: the tiled kernels without the fused
    last pass."""
    by_name = {c[0]: c for c in CIRCUITS}
    ops = tm.compile_gates(sc.N, by_name["flip_xor3_aligned4"][3])[0]
    assert all(tm.op_is_pair(o.kind) for o in ops[:4]) and ops[3].xm == ops[0].xm ^ ops[1].xm ^ ops[2].xm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "child.py"
    script.write_text("import sys\nsys.path[:0] = %r\nimport test_stream_planner_gpu as t\nt.child_main()\n"
                      % ([root, os.path.join(root, "oracle"), os.path.join(root, "tests")],))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, **{switch: "0"}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("%s=0: %d cases, worst amplitude error %.2e, worst energy error %.2e" % (switch, out["cases"], out["amplitude"], out["energy"]))
    assert out["cases"] >= 45 and out["amplitude"] < A_TOL and out["energy"] < E_TOL
