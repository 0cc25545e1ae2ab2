#!/usr/bin/env python3
"""Benchmark of the VQE environment-step hot path (BASELINE.json metric: VQE env-steps/sec).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One bench *step* = one CircuitEnv.step() worth of arithmetic for every one of the B parallel
environments of a rank, in one fused launch: COBYLA (scipy-1.15 defaults rhobeg=1, rhoend=1e-4,
maxfun=1000) on the pre-action circuit, float32 round-trip of the angles, energy of the
post-action circuit (reference environments/environment_qulacs_TN_notin_agent.py:283-291).

Workload (SURVEY.md section 8d, config "12-qubit LiH TensorRL_fixed noiseless"): SYNTHETIC
LiH-like 631-term Pauli Hamiltonian (the reference never shipped LiH-12q), brickwork chi=2
stand-in initial state, random circuits of G gates (half CNOTs, half R{X,Y,Z}, theta ~
U(-pi, pi) rounded to float32), the last gate being the "new" one.  Inputs are resident in
HBM before the timed region and are not modified by a step, so every step does identical
work.  Multi-GPU: environments are sharded over ranks (replicas, no data-path collective,
weak scaling); the auxiliary ``heis20`` object times the 20-qubit Heisenberg <H> with Pauli
terms sharded over the ranks and ONE RCCL all-reduce of the partial energies.

A plain run sets up, warms up, times the --steps launches of the headline kernel and prints the JSON line
(`value` env-steps/s over all ranks, `ms_per_step` wall milliseconds of one timed step).  --full adds the
auxiliary objects (warm start, gate sweep, noisy / trainable / exact-channel launches, the episodes, heis20,
the MPS -> PQC fits and the CPU baselines).  --dump-outputs DIR writes what the last timed step returned to
its caller (per-environment energies, optimised angles and evaluation counts) as DIR/<name>.npy in float64;
the inputs are seeded, so two builds can be compared output for output.

Launch: under torchrun (RANK / LOCAL_RANK / WORLD_SIZE in the environment) every process is one rank.
Started plainly with --gpus N > 1 and no WORLD_SIZE, this process spawns the N ranks itself
(`python -m torch.distributed.run ...` as a child, before anything here touches the GPU) and exits
with the child's code; the JSON line carries `ranks_seen` = torch.distributed's world size.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_QUBITS = 12
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def make_batch(tq, n, B, G, seed):
    """B random circuits of G gates (SURVEY 8d generator), vectorised."""
    rng = np.random.default_rng(seed)
    is_cnot = rng.random((B, G)) < 0.5
    c = rng.integers(0, n, (B, G))
    t = (c + 1 + rng.integers(0, n - 1, (B, G))) % n
    rq = rng.integers(0, n, (B, G))
    rk = rng.integers(1, 4, (B, G))
    kind = np.where(is_cnot, 0, rk).astype(np.int32)
    q0 = np.where(is_cnot, c, rq).astype(np.int32)
    q1 = np.where(is_cnot, t, -1).astype(np.int32)
    rot = ~is_cnot
    pidx = np.where(rot, np.cumsum(rot, axis=1) - 1, -1).astype(np.int32)
    pcount = rot.sum(axis=1)
    gate_off = np.arange(B + 1, dtype=np.int64) * G
    par_off = np.concatenate([[0], np.cumsum(pcount)]).astype(np.int64)
    theta = rng.uniform(-np.pi, np.pi, int(par_off[-1])).astype(np.float32).astype(np.float64)
    # the new gate is the last one; a new rotation enters with angle 0 (reference step())
    last_rot = rot[:, -1]
    theta[par_off[1:][last_rot] - 1] = 0.0
    new_gate = np.full(B, G - 1, np.int32)
    return dict(gate_off=gate_off, kind=kind.ravel(), q0=q0.ravel(), q1=q1.ravel(), pidx=pidx.ravel(),
                par_off=par_off, theta=theta, new_gate=new_gate, pcount=pcount)


def _cpu_facts():
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    blas = ""
    try:
        from threadpoolctl import threadpool_info
        blas = "; ".join(f"{p.get('internal_api')} {p.get('version')} ({p.get('num_threads')} threads)"
                         for p in threadpool_info() if p.get("user_api") == "blas")
    except Exception:
        pass
    return model, blas


ALL_CPUS = None      # the CPU mask of the process before main() bound its host threads


def cpu_baseline(tq, ham, psi0, batch, G, n_steps, maxfun, one_thread_evals=400):
    """Reference algorithm on the host cores for a bounded sample of the same workload:
    C restatement of the qulacs gate sweeps (oracle/vqe_oracle.c) + the literal dense
    numpy expression (VQE_qulacs_TN_notin_RL.py:86) inside scipy's COBYLA (:478).
    Timed twice: with the BLAS pool at all host cores (`value`: whole env-steps) and at ONE thread
    (the reference pins torch to one thread, TensorRL_fixed_noiseless.py:13; qulacs' small-n kernels are
    single-threaded): there a bounded number of evaluations of the same COBYLA run, converted with the
    workload's evaluations per env-step."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import c_oracle as co
    import vqe_oracle as vo
    from scipy.optimize import minimize
    from threadpoolctl import threadpool_limits
    # the CPU reference gets every core of the host: main() confined this thread to one L3 domain for the GPU's sake
    if ALL_CPUS is not None and hasattr(os, "sched_setaffinity"):
        os.sched_setaffinity(0, ALL_CPUS)
    n = N_QUBITS
    idx = np.arange(2 ** n)
    dense = np.zeros((2 ** n, 2 ** n), np.complex128)
    for x, z, w in zip(ham.xmask, ham.zmask, ham.coeff):
        x, z = int(x), int(z)
        ny = bin(x & z).count("1")
        dense[idx ^ x, idx] += w * (1.0 - 2.0 * vo._parity(idx & z)) * (1j ** ny)
    nproc = os.cpu_count() or 1
    try:
        nproc = len(os.sched_getaffinity(0))
    except AttributeError:
        pass
    model, blas = _cpu_facts()

    def env_step(b, budget=None):
        """One CircuitEnv.step() of circuit b on the CPU; `budget`: stop after that many evaluations."""
        g0, g1 = batch["gate_off"][b], batch["gate_off"][b + 1]
        p0, p1 = batch["par_off"][b], batch["par_off"][b + 1]
        kind, q0, q1, pidx = (batch[k][g0:g1] for k in ("kind", "q0", "q1", "pidx"))
        th = batch["theta"][p0:p1].copy()
        pre = slice(0, G - 1)
        hole = int(pidx[-1])
        x0 = th if hole < 0 else th[:hole]          # the new rotation is the last parameter
        count = [0]

        class Budget(Exception):
            pass

        def cost(x, k=kind[pre], a=q0[pre], bq=q1[pre], p=pidx[pre]):
            if budget is not None and count[0] >= budget:
                raise Budget
            count[0] += 1
            psi = co.run_circuit(n, psi0, k, a, bq, p, x)
            return float((np.conj(psi).T @ dense @ psi).real)

        try:
            r = minimize(cost, x0, method="COBYLA", options={"maxiter": maxfun})
        except Budget:
            return count[0]
        full = th.copy()
        full[:x0.size] = r.x.astype(np.float32)
        psi = co.run_circuit(n, psi0, kind, q0, q1, pidx, full)
        _ = float((np.conj(psi).T @ dense @ psi).real)
        return r.nfev + 1

    evals = 0
    t0 = time.perf_counter()
    with threadpool_limits(limits=nproc, user_api="blas"):
        for b in range(n_steps):
            evals += env_step(b)
    dt = time.perf_counter() - t0
    per_step = evals / n_steps
    with threadpool_limits(limits=1, user_api="blas"):
        t1 = time.perf_counter()
        e1 = env_step(0, budget=one_thread_evals)
        d1 = time.perf_counter() - t1
    return {"value": n_steps / dt, "unit": "env-steps/s", "cores": int(nproc), "kind": "port",
            "sample": f"{n_steps} env-steps of the same batch ({evals} evaluations, {dt:.1f} s), BLAS pool at {nproc} threads: "
                      f"C gate sweeps + numpy dense (conj(psi)@H)@psi + scipy {__import__('scipy').__version__} COBYLA",
            "evals_per_s": evals / dt,
            "one_thread": {"value": (e1 / d1) / per_step, "unit": "env-steps/s", "cores": 1, "evals_per_s": e1 / d1,
                           "sample": f"first {e1} evaluations of env-step 0 ({d1:.1f} s) at 1 BLAS thread, converted with "
                                     f"{per_step:.0f} evaluations per env-step of this workload"},
            "nproc": int(nproc), "cpu_model": model, "blas": blas}


def episode_aux(tq, torch, dev, num_envs, max_steps, barrier=None, seed0=0, native=True):
    """The named configuration itself: TensorRL_fixed/LIH12q_TNbond2 (137 layers, 110 steps per
    episode, COBYLA maxiter 1000) through VecCircuitEnv - the env.step() / reset() surface the DeepQ
    driver calls - with a uniformly random legal policy: warm-started COBYLA exactly as in the
    reference's episodes.  Data are the synthetic LiH-12q stand-ins (tensorrl_qas_amd.synthetic).
    Host side: the compiled loop of csrc/vec_env.cpp (one Python process); two half batches are software
    pipelined (step_async / step_wait: the host work of one overlaps the launch of the other).
    Reports the wall rate and the rate of the device part alone."""
    import copy
    import tempfile
    from tensorrl_qas_amd import synthetic
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    root = synthetic.write_lih12_dataset(tempfile.mkdtemp(prefix="lih12_"))
    conf = copy.deepcopy(synthetic.LIH12_FIXED_CONFIG)
    conf["env"]["data_root"] = root
    half = max(1, num_envs // 2)
    vecs = [VecCircuitEnv(CircuitEnv, conf, torch.device(f"cuda:{dev}"), half, seed=s, native=native) for s in (seed0, seed0 + 1)]
    num_envs = 2 * half
    tdict = vecs[0]._proto._actions_table
    table = np.array([tdict[i] for i in range(len(tdict))], np.int32)
    rng = np.random.default_rng(7 + seed0)
    for v in vecs:
        v.reset()
    n_steps = min(max_steps, vecs[0]._proto.num_layers_termination)
    steps = nfev = 0
    t_gpu = 0.0

    def choose(vec):
        """uniformly random LEGAL action per environment (illegal_action_new() of every environment first,
        as the reference's driver does before each step, TensorRL_fixed_noiseless.py:118-120)"""
        if vec.native:
            ill = vec.illegal_actions_array()
        else:
            lists = vec.illegal_actions()
            ill = np.full((vec.num_envs, vec.num_qubits), -1, np.int32)
            for b, l in enumerate(lists):
                ill[b, :len(l)] = l
        a = rng.integers(0, table.shape[0], vec.num_envs)
        bad = (ill == a[:, None]).any(axis=1)
        while bad.any():
            a[bad] = rng.integers(0, table.shape[0], int(bad.sum()))
            bad = (ill == a[:, None]).any(axis=1)
        return table[a]

    def collect(vec):
        nonlocal steps, nfev, t_gpu
        vec.step_wait()
        t_gpu += vec.engine.last_kernel_ms() * 1e-3
        steps += vec.num_envs
        nfev += float(np.sum(vec.nfev))

    if barrier is not None:      # tools/probe_episode_procs.py: several host processes share the GPU
        barrier.wait()
    t_start = time.time()
    t0 = time.perf_counter()
    vecs[0].step_async(choose(vecs[0]))
    for it in range(n_steps):
        vecs[1].step_async(choose(vecs[1]))          # launch B while A runs
        collect(vecs[0])
        if it + 1 < n_steps:
            vecs[0].step_async(choose(vecs[0]))      # launch A's next step while B runs
        collect(vecs[1])
    dt = time.perf_counter() - t0
    rot = [float(np.mean(v._field("n_rotations"))) if v.native else
           float(np.mean([int((e.state[:, 12:15] == 1).sum()) for e in v.envs])) for v in vecs]
    return {"workload": f"TensorRL_fixed/LIH12q_TNbond2 (synthetic data), 2 x {half} envs x {n_steps} steps, random legal policy, "
                        "half batches pipelined (step_async / step_wait), ONE host process",
            "host_loop": "native (csrc/vec_env.cpp)" if vecs[0].native else "python objects",
            "env_steps_per_s_wall": steps / dt, "env_steps_per_s_device": steps / t_gpu,
            "env_steps": steps, "t_start": t_start, "t_end": t_start + dt,
            "device_note": "sum of the kernel times of both halves; their launches may overlap on the GPU",
            "mean_nfev_per_step": nfev / steps, "mean_rotations_at_end": float(np.mean(rot))}


FP64_PEAK_TFLOPS = 78.6   # MI355X FP64, vector = matrix rate (half of the guide's 157.3 TF FP32 vector figure)


def mps2qc_aux(tq, dev, with_cpu):
    """Offline MPS -> PQC fit (reference dmrg-to-qc/mps2qc.py + stiefel_opt.py): 1024
    random restarts of a 12-qubit one-layer brickwork (11 SU(4) gates) fitted to one random target for 200
    Stiefel-Adam steps in ONE launch of k_fit<12,512>.  Algorithmic flops per optimiser step:
    G forward + 2G backward gate sweeps + G environments, each 2^n * 32 flop (16 complex MACs per 4 amplitudes)."""
    from tensorrl_qas_amd import dmrg_to_qc as dq
    n, layers, B, iters = 12, 1, 1024, 200
    rng = np.random.default_rng(1212)
    sites, G = dq.brickwork_ansatz(n, layers)
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    target = v / np.linalg.norm(v)
    init = np.array([[dq.rand_uni(4, rng) for _ in range(G)] for _ in range(B)])
    opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=True, device_id=dev)
    prob = dq.BrickworkOverlap(n, sites, target)
    opt.minimize(prob, init, max_iter=iters, tol=0.0, param_tol=0.0)       # warm-up launch
    opt.minimize(prob, init, max_iter=iters, tol=0.0, param_tol=0.0)
    steps = int(np.sum(opt.n_iter))
    flop = steps * 4 * G * (1 << n) * 32
    tf = flop / (opt.kernel_ms * 1e-3) / 1e12
    out = {"workload": f"brickwork_fit_{n}q_{layers}layer_G{G}_B{B}_iters{iters}_random_target",
           "optimiser_steps_per_s": steps / (opt.kernel_ms * 1e-3), "fits_per_s": B / (opt.kernel_ms * 1e-3),
           "kernel": "k_fit<12,512>", "kernel_ms": opt.kernel_ms, "mean_final_loss": float(np.mean(
               [h[-1] for h in opt.loss_history])), "dtype": "f64",
           "roofline": {"bound": "mfma", "achieved": tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": tf / FP64_PEAK_TFLOPS, "traffic": None,
                        "algorithmic_flop_per_step": 4 * G * (1 << n) * 32,
                        "note": "environments on v_mfma_f64_16x16x4_f64, gate sweeps on FP64 vector FMAs; "
                                "both pipes peak at the same 78.6 TFLOP/s on MI355X; states LDS-resident"}}
    pm, why = load_pmc("mps2qc", out["workload"])      # HBM bytes per launch from separate rocprofv3 --pmc passes
    if pm is not None and "FETCH_SIZE" in pm.get("per_launch", {}) and "WRITE_SIZE" in pm["per_launch"]:
        out["roofline"]["traffic"] = (2.0 * pm["per_launch"]["FETCH_SIZE"] + pm["per_launch"]["WRITE_SIZE"]) * 1024.0
        out["roofline"]["traffic_source"] = pm.get("source")
    else:
        out["roofline"]["traffic_note"] = why
    if with_cpu:      # the numpy restatement (oracle/stiefel_oracle.py) on one fit, a few steps
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import stiefel_oracle as so
        ref = so.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=True)
        ref.init(init[0])
        t0 = time.perf_counter()
        _, _, hist, _ = ref.minimize(n, list(sites), target, init[0], max_iter=40, tol=0.0, param_tol=0.0)
        dt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": len(hist) / dt, "unit": "optimiser steps/s", "cores": 1, "kind": "port",
                               "sample": "40 steps of one fit, numpy restatement (the reference runs jax + quimb)",
                               "max_abs_loss_diff_vs_gpu": float(np.max(np.abs(
                                   np.array(hist) - np.array(opt.loss_history[0][:len(hist)]))))}
    return out


def heis20_aux(tq, torch, dist, rank, world, dev, steps):
    """20-qubit Heisenberg <H>: every rank applies the same circuits, evaluates its share of
    the X-mask groups, one all-reduce (RCCL) sums the partial energies.  Strong scaling of
    the Pauli-term reduction."""
    n, B, G = 20, 256, 32      # B evaluations per all-reduce (>= 64; 4 GiB of states)
    ham, _ = tq.hamiltonian.heisenberg(n)
    eng = tq.VQEEngine(n, dev)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    # initial state: the package's own chi = 2-like init circuit for this chain (Lanczos ground state -> streaming MPS-to-PQC
    # fit -> {rz, ry, cx} text, tools/make_heis20_init.py; |<gs|init>|^2 = 0.59, E = -33.56 against E0 = -36.01)
    init_file = os.path.join(ROOT, "tensorrl-qas_amd", "data", "init_heisenberg_20q_TNbond2.qasm")
    init_note = "|0...0>"
    if os.path.exists(init_file):
        ic, iang = tq.circuits.circuit_from_qasm_gates(tq.qasm.parse(open(init_file).read())[1])
        eng.set_circuit(ic)
        eng.set_init_state(eng.get_state(iang))
        init_note = "tensorrl-qas_amd/data/init_heisenberg_20q_TNbond2.qasm (own fit of the Lanczos ground state)"
    eng.set_amplitude_shard(rank, world)     # every rank: all 77 terms on 1/world of the basis states
    batch = make_batch(tq, n, B, G, 2020)
    eng.batch_load_flat(batch["gate_off"], batch["kind"], batch["q0"], batch["q1"], batch["pidx"],
                        batch["par_off"], batch["theta"])
    e = torch.zeros(B, dtype=torch.float64, device=f"cuda:{dev}")

    def one():
        eng.batch_run_energy()
        eng.batch_copy_energy(e.data_ptr())
        if world > 1:
            dist.all_reduce(e)

    one()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the Pauli-term reduction alone (this rank's X-mask groups + the all-reduce), states resident
    def red():
        eng.batch_run_reduction()
        eng.batch_copy_energy(e.data_ptr())
        if world > 1:
            dist.all_reduce(e)

    red()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    for _ in range(steps):
        red()
    torch.cuda.synchronize()
    dr = time.perf_counter() - t1
    t = torch.tensor([dt, dr], dtype=torch.float64, device=f"cuda:{dev}")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    # algorithmic bytes of one evaluation: 2^n * 16 * (2 G_rot + T_x), G_rot = mean rotations per circuit
    g_rot = float(np.count_nonzero(batch["kind"])) / B
    bytes_per_eval = (1 << n) * 16 * (2 * g_rot + 20)
    evals_s = B * steps / float(t[0].item())
    roof = {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None,
            "note": "no profiles/pmc_heis20.json for this workload (tools/pmc_heis20.sh)"}
    tfile = os.path.join(ROOT, "profiles", "pmc_heis20.json")
    if os.path.exists(tfile):      # HBM bytes of one batched evaluation from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes
        tr = json.load(open(tfile))
        if tr.get("workload") == "heisenberg_20q_77terms_G32_B256_sharded" and tr.get("src_sha16") != src_sha16():
            roof["note"] = f"profiles/pmc_heis20.json was measured on other sources ({tr.get('src_sha16')}): re-run tools/pmc_heis20.sh"
        elif tr.get("workload") == "heisenberg_20q_77terms_G32_B256_sharded":
            per_batch = tr["hbm_bytes_per_batch"]
            gbs = per_batch * (evals_s / B) / 1e9
            roof = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                    "traffic": per_batch, "traffic_source": tr["source"],
                    "note": "measured HBM bytes of one batch of 256 evaluations (all k_t_* / k_s_* launches, one GPU) x batches/s of "
                            "this run; at N > 1 every rank moves the circuit part again, so this is the per-GPU figure at N = 1"}
            # per kernel: bytes and duration of the same profiled batch (rocprofv3 --stats pass of tools/pmc_heis20.sh)
            roof["kernels"] = {k: {"bound": "hbm", "achieved": v["GBs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                   "frac": (v["GBs"] / HBM_PEAK_GBS) if v.get("GBs") else None, "traffic": v["hbm_bytes_per_batch"],
                                   "ms_per_batch": v["ms_per_batch"], "launches_per_batch": v["launches_per_batch"]}
                               for k, v in tr.get("kernels", {}).items() if v.get("ms_per_batch") and ("k_t_ops" in k or "k_t_energy" in k)}
    roof["algorithmic"] = {"bytes_per_evaluation": bytes_per_eval, "mean_rotations": g_rot,
                           "GBs_if_every_gate_and_group_streamed": bytes_per_eval * evals_s / 1e9,
                           "note": "SURVEY 8d figure 2^n*16*(2 G_rot + T_x): informational - the LDS-tiled kernels apply several "
                                   "ops / groups per pass over the state"}
    return {"workload": "heisenberg_20q_77terms_G32_B256_sharded", "init_state": init_note, "evals_per_s": evals_s,
            "roofline": roof,
            "reduction_ms_per_batch": float(t[1].item()) / steps * 1e3,
            "reduction_evals_per_s": B * steps / float(t[1].item()),
            "x_groups_total": 20, "sharding": "amplitude slices (tiles) of the term sum, 1 all-reduce", "energy_checksum": float(e.sum().item()), "scaling": "strong"}


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as children of this process
    (torchrun's elastic launcher), BEFORE anything here initialises the GPU - a process that has touched
    the GPU must never be replaced or forked into ranks.  Returns the child's exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this pool (RCCL across processes)
    return subprocess.call(cmd, env=env)


def launch_selftest(args, rank, world):
    """CPU rehearsal of the multi-rank launch path (tests/test_distributed_cpu.py): rendezvous, one
    all-reduce, rank 0 prints the JSON line - no GPU work."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if world > 1:
        dist.init_process_group(args.backend, rank=rank, world_size=world)
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t)
    if rank == 0:
        print(json.dumps({"selftest": True, "n_gpus": args.gpus, "ranks_seen": dist.get_world_size() if world > 1 else 1,
                          "backend": args.backend if world > 1 else None, "rank_sum": float(t.item())}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


DUMP_BUDGET = 60 * 10 ** 6      # array bytes written by --dump-outputs (index arrays of samples included): < 64 MB with headers


def dump_outputs(out_dir, arrays, rank, world):
    """--dump-outputs: one float64 .npy per array (suffixed with the rank when there are several).  Should the arrays
    outgrow DUMP_BUDGET, every array is replaced by the same fraction of its entries, drawn with a fixed seed, and
    <name>_index.npy records which entries those are."""
    os.makedirs(out_dir, exist_ok=True)
    sfx = f"_rank{rank}" if world > 1 else ""
    arrays = {k: np.asarray(v, np.float64).ravel() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    keep = 1.0 if total <= DUMP_BUDGET else DUMP_BUDGET / (2.0 * total)      # value + index per sampled entry
    for name, a in arrays.items():
        if keep < 1.0:
            idx = np.sort(np.random.default_rng(0).choice(a.size, max(1, int(a.size * keep)), replace=False))
            np.save(os.path.join(out_dir, f"{name}_index{sfx}.npy"), idx.astype(np.float64))
            a = a[idx]
        np.save(os.path.join(out_dir, f"{name}{sfx}.npy"), a)


def src_sha16():
    """Hash of the kernel sources: a counter file describes ONE build (instruction counts are properties of the code),
    so every profiles/pmc_*.json carries the hash of the sources it was measured on and is ignored when they moved on."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "tensorrl-qas_amd", "csrc")
    # the DEVICE sources and the build flags (vqe_api.hip and vec_env.cpp are host code: launch plumbing, planners)
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith(".h") or fn in ("mps2qc_fit.hip", "Makefile"):
            h.update(fn.encode())
            h.update(open(os.path.join(csrc, fn), "rb").read())
    return h.hexdigest()[:16]


def load_pmc(key, workload):
    """profiles/pmc_<key>.json (tools/pmc_collect.py: rocprofv3 --pmc passes over `bench.py --only <key>`) when it
    belongs to this workload AND to the current sources; else (None, reason)."""
    path = os.path.join(ROOT, "profiles", f"pmc_{key}.json")
    if not os.path.exists(path):
        return None, f"no profiles/pmc_{key}.json (tools/pmc_collect.py {key})"
    try:
        pm = json.load(open(path))
    except ValueError:
        return None, f"profiles/pmc_{key}.json is not valid JSON"
    if pm.get("workload") != workload:
        return None, f"profiles/pmc_{key}.json describes another workload ({pm.get('workload')})"
    if pm.get("src_sha16") != src_sha16():
        return None, f"profiles/pmc_{key}.json was measured on other sources ({pm.get('src_sha16')}, now {src_sha16()}): re-run tools/pmc_collect.py {key}"
    return pm, None


def counter_roofline(key, workload, kernel, k_ms, bound="fp64_valu", waves_per_unit=None, units_per_launch=None):
    """Roofline object of one kernel from its counter file and the duration measured live in this run (HIP events).
    fp64_valu: executed FP64 vector flops (2 FMA + MUL + ADD wave instructions x 64 lanes) / time against the 78.6 TFLOP/s
    FP64 peak; hbm: measured HBM bytes ((2 FETCH_SIZE + WRITE_SIZE) x 1024, gfx950 read correction) / time against 8 TB/s.
    Every missing counter is reported, never guessed."""
    pm, why = load_pmc(key, workload)
    peak, unit = (FP64_PEAK_TFLOPS, "TFLOP/s") if bound == "fp64_valu" else (HBM_PEAK_GBS, "GB/s")
    out = {"bound": bound, "achieved": None, "peak": peak, "unit": unit, "frac": None, "traffic": None, "kernel": kernel,
           "kernel_ms": k_ms}
    if pm is None:
        out["note"] = why
        return out
    c = pm.get("per_launch", {})
    sec = k_ms * 1e-3
    need = ("SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_ADD_F64")
    flop = (2.0 * c[need[0]] + c[need[1]] + c[need[2]]) * 64.0 if all(k in c for k in need) else None
    hbm = (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0 if "FETCH_SIZE" in c and "WRITE_SIZE" in c else None
    out["source"] = pm.get("source")
    out["kernel_ms_under_rocprof"] = pm.get("kernel_ms_avg")
    out["traffic"] = hbm
    missing = [k for k in need if k not in c] if bound == "fp64_valu" else [k for k in ("FETCH_SIZE", "WRITE_SIZE") if k not in c]
    if missing:
        out["note"] = "counter file lacks " + ", ".join(missing)
        return out
    if bound == "fp64_valu":
        out.update(achieved=flop / sec / 1e12, frac=flop / sec / 1e12 / FP64_PEAK_TFLOPS, flop_per_launch=flop)
        if hbm is not None:
            out["hbm"] = {"achieved": hbm / sec / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hbm / sec / 1e9 / HBM_PEAK_GBS}
    else:
        out.update(achieved=hbm / sec / 1e9, frac=hbm / sec / 1e9 / HBM_PEAK_GBS)
        if flop is not None:
            out["fp64"] = {"achieved": flop / sec / 1e12, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": flop / sec / 1e12 / FP64_PEAK_TFLOPS}
    if units_per_launch:
        out["flop_per_evaluation" if bound == "fp64_valu" else "bytes_per_unit"] = (flop if bound == "fp64_valu" else hbm) / units_per_launch
    if c.get("SQ_INSTS_ALL") and c.get("SQ_WAVE_CYCLES") and waves_per_unit and units_per_launch:
        waves = float(waves_per_unit) * units_per_launch
        f64 = sum(c.get(k, 0.0) for k in need)
        out["issue"] = {"wave_instructions_per_evaluation": c["SQ_INSTS_ALL"] / waves, "of_which_fp64_valu": f64 / waves,
                        "of_which_valu": c.get("SQ_INSTS_VALU", 0.0) / waves,
                        "fp64_share_of_wave_instructions": f64 / c["SQ_INSTS_ALL"],
                        "wave_cycles_instruction_active": c.get("SQ_ACTIVE_INST_ANY", 0.0) / c["SQ_WAVE_CYCLES"],
                        "wave_cycles_waiting_on_counter": c.get("SQ_WAIT_ANY", 0.0) / c["SQ_WAVE_CYCLES"],
                        "wave_cycles_waiting_for_issue": c.get("SQ_WAIT_INST_ANY", 0.0) / c["SQ_WAVE_CYCLES"]}
    if "SQ_LDS_IDX_ACTIVE" in c and "GRBM_GUI_ACTIVE" in c and c["GRBM_GUI_ACTIVE"]:
        cus, xcds = pm.get("cu_count", 256), pm.get("xcd_count", 8)   # GRBM_GUI_ACTIVE is summed over the XCDs, SQ_* over all CUs
        out["lds"] = {"array_cycles_per_launch": c["SQ_LDS_IDX_ACTIVE"], "bank_conflict_cycles": c.get("SQ_LDS_BANK_CONFLICT"),
                      "frac": c["SQ_LDS_IDX_ACTIVE"] / (cus * c["GRBM_GUI_ACTIVE"] / xcds)}
        if "SQ_INSTS_VALU" in c:
            out["valu_busy_frac"] = 4.0 * c["SQ_INSTS_VALU"] / (4.0 * cus * c["GRBM_GUI_ACTIVE"] / xcds)   # 4 cycles per wave64 VALU op, 4 SIMDs per CU
    return out


def g_sweep(tq, eng, n, B, maxfun, rank):
    """RL-depth sweep G in {8, 32, 64, 110} of the same generator, one fused launch each."""
    out = []
    for G in (8, 32, 64, 110):
        b = make_batch(tq, n, B, G, 1000 + rank)
        eng.batch_load_flat(b["gate_off"], b["kind"], b["q0"], b["q1"], b["pidx"], b["par_off"], b["theta"])
        eng.batch_set_new_gate(b["new_gate"])
        eng.batch_run_env_step(1.0, 1e-4, maxfun)
        eng.sync()
        ms = eng.last_kernel_ms()
        _, _, nfev = eng.batch_fetch(want_x=False)
        out.append({"gates": G, "mean_params": float(np.mean(b["pcount"])), "env_steps_per_s_per_gpu": B / (ms * 1e-3),
                    "evals_per_s_per_gpu": float(nfev.sum() + B) / (ms * 1e-3), "mean_nfev": float(nfev.mean()), "kernel_ms": ms})
    return out


def episode8_aux(tq, torch, dev, num_envs=8192):
    """The configuration the reference ships most often: TensorRL_fixed/H2O8q_TNbond2 - the shipped 193-term Hamiltonian
    and chi = 2 init circuit (fixtures under tests/golden/: data of the reference, with the parsed config), 20 steps per
    episode - through VecCircuitEnv with the compiled host loop, uniformly random legal actions, two half batches
    software pipelined, one process.  (configuration_files/TensorRL_fixed/H2O8q_TNbond2.cfg of the reference)"""
    import tempfile
    from tensorrl_qas_amd.environments.environment_qulacs_TN_notin_agent import CircuitEnv
    from tensorrl_qas_amd.environments.vec_env import VecCircuitEnv
    gold = os.path.join(ROOT, "tests", "golden")
    conf = json.load(open(os.path.join(gold, "host_logic.json")))["configs"]["TensorRL_fixed/H2O8q_TNbond2"]
    conf = json.loads(json.dumps(conf))
    root = tempfile.mkdtemp(prefix="h2o8_")
    os.makedirs(os.path.join(root, "mol_data"))
    os.makedirs(os.path.join(root, "init_state_circ"))
    stem = "H2O_8q_geom_H_-0.021_-0.002_0.000;_O_0.835_0.452_0.000;_H_1.477_-0.273_0.000_jordan_wigner"
    d = np.load(os.path.join(gold, "ham_H2O_8q.npz"))
    np.savez(os.path.join(root, "mol_data", stem + ".npz"), paulis=np.array([str(x) for x in d["paulis"]]),
             weights=np.asarray(d["weights"], float), eigvals=np.asarray(d["eigvals"], float), energy_shift=0)
    names = {0: "cx", 1: "rx", 2: "ry", 3: "rz"}
    lines = ["OPENQASM 2.0;", 'include "qelib1.inc";', f"qreg q[{int(d['n'])}];"]
    for nm, a, bq, ang in zip(d["gate_name"], d["gate_q0"], d["gate_q1"], d["gate_angle"]):
        lines.append(f"cx q[{int(a)}],q[{int(bq)}];" if int(nm) == 0 else f"{names[int(nm)]}({float(ang)!r}) q[{int(a)}];")
    with open(os.path.join(root, "init_state_circ", f"init_{stem}_TNbond2.qasm"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    conf["env"]["data_root"] = root
    half = max(1, num_envs // 2)
    vecs = [VecCircuitEnv(CircuitEnv, conf, torch.device(f"cuda:{dev}"), half, seed=s, native=True) for s in (0, 1)]
    tdict = vecs[0]._proto._actions_table
    table = np.array([tdict[i] for i in range(len(tdict))], np.int32)
    rng = np.random.default_rng(7)
    for v in vecs:
        v.reset()
    n_steps = vecs[0]._proto.num_layers_termination

    def choose(vec):
        ill = vec.illegal_actions_array()
        a = rng.integers(0, table.shape[0], vec.num_envs)
        bad = (ill == a[:, None]).any(axis=1)
        while bad.any():
            a[bad] = rng.integers(0, table.shape[0], int(bad.sum()))
            bad = (ill == a[:, None]).any(axis=1)
        return table[a]

    steps = 0
    nfev = t_gpu = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vecs[0].step_async(choose(vecs[0]))
    for it in range(n_steps):
        vecs[1].step_async(choose(vecs[1]))
        for k in (0, 1):
            vecs[k].step_wait()
            t_gpu += vecs[k].engine.last_kernel_ms() * 1e-3
            steps += half
            nfev += float(np.sum(vecs[k].nfev))
            if k == 0 and it + 1 < n_steps:
                vecs[0].step_async(choose(vecs[0]))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    err = np.concatenate([v.errors for v in vecs])
    return {"config": "TensorRL_fixed/H2O8q_TNbond2 (shipped Hamiltonian and init circuit)", "envs": 2 * half,
            "steps_per_episode": int(n_steps), "env_steps": steps, "env_steps_per_s_wall": steps / dt,
            "env_steps_per_s_device": steps / t_gpu, "mean_nfev": nfev / steps, "final_error_min_Ha": float(err.min()),
            "host_loop": "native (csrc/vec_env.cpp), one process, two half batches pipelined"}


def noisy_aux(tq, n, ham, psi0, batch, B, G, maxfun):
    """BASELINE config 5 at bench size: the same circuits with a depolarising channel behind every gate
    (p1 = 0.01, p2 = 0.05; reference environments/VQAs/VQE_qulacs_TN_notin_RL_noise.py:13-54), one Pauli
    trajectory per evaluation, fused env-step kernel.  A noisy objective ends COBYLA early, so env-steps/s
    and evaluations/s are both given."""
    k = batch["kind"].reshape(B, G); q0 = batch["q0"].reshape(B, G); q1 = batch["q1"].reshape(B, G)
    p = batch["pidx"].reshape(B, G)
    k2 = np.empty((B, 2 * G), np.int32); a2 = np.empty_like(k2); b2 = np.empty_like(k2); p2 = np.empty_like(k2)
    k2[:, 0::2] = k; k2[:, 1::2] = np.where(k == 0, 5, 4)          # DEPOL2 behind a CNOT, DEPOL1 behind a rotation
    a2[:, 0::2] = q0; a2[:, 1::2] = q0
    b2[:, 0::2] = q1; b2[:, 1::2] = np.where(k == 0, q1, -1)
    p2[:, 0::2] = p; p2[:, 1::2] = -1
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    eng.set_noise(0.01, 0.05, 7)
    eng.batch_load_flat(np.arange(B + 1, dtype=np.int64) * 2 * G, k2.ravel(), a2.ravel(), b2.ravel(), p2.ravel(),
                        batch["par_off"], batch["theta"])
    eng.batch_set_new_gate(np.full(B, 2 * G - 2, np.int32))
    for _ in range(2):
        eng.batch_run_env_step(1.0, 1e-4, maxfun)
        eng.sync()
    ms = eng.last_kernel_ms()
    _, f, nfev = eng.batch_fetch(want_x=False)
    workload = f"lih12_synthetic631_fixed_noise_p1_0.01_p2_0.05_G{G}_B{B}"
    evals = float(nfev.sum() + B)
    return {"workload": workload, "env_steps_per_s_per_gpu": B / (ms * 1e-3),
            "evals_per_s_per_gpu": evals / (ms * 1e-3), "mean_nfev": float(nfev.mean()), "kernel_ms": ms,
            "mean_energy": float(np.mean(f)), "noise": "Pauli trajectories, one draw per (environment, evaluation, gate)",
            "roofline": counter_roofline("noisy12", workload, "k_lds_minimize<12, false, true>", ms, "fp64_valu", 4, evals)}


def trainable8_aux(tq, B=4096, G=150, maxfun=300):
    """BASELINE config 2 regime: 8-qubit H2O (the shipped 193-term Hamiltonian), circuits of the size the trainable
    path starts from (150 gates, ~129 rotations, all of them variables; reference environment_qulacs.py:285-328),
    from |0...0>, fused minimisation with maxfun 300: the optimiser's 2 x 137^2 matrices live in L2 here and its
    update is most of an evaluation."""
    n = 8
    ham = tq.hamiltonian.load_npz(os.path.join(ROOT, "tests", "golden", "ham_H2O_8q.npz"), n)
    rng = np.random.default_rng(0)
    kind = np.where(rng.random((B, G)) < 0.14, 0, rng.integers(1, 4, (B, G))).astype(np.int32)
    c = rng.integers(0, n, (B, G))
    t = (c + 1 + rng.integers(0, n - 1, (B, G))) % n
    q0 = np.where(kind == 0, c, rng.integers(0, n, (B, G))).astype(np.int32)
    q1 = np.where(kind == 0, t, -1).astype(np.int32)
    rot = kind != 0
    pidx = np.where(rot, np.cumsum(rot, axis=1) - 1, -1).astype(np.int32)
    par_off = np.concatenate([[0], np.cumsum(rot.sum(1))]).astype(np.int64)
    theta = rng.uniform(-np.pi, np.pi, int(par_off[-1]))
    eng = tq.VQEEngine(n)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    eng.batch_load_flat(np.arange(B + 1, dtype=np.int64) * G, kind.ravel(), q0.ravel(), q1.ravel(), pidx.ravel(), par_off, theta)
    for _ in range(2):
        eng.batch_run_minimize(1.0, 1e-4, maxfun)
        eng.sync()
    ms = eng.last_kernel_ms()
    _, f, nfev = eng.batch_fetch(want_x=False)
    workload = f"h2o8_193terms_trainable_regime_G{G}_P{rot.sum(1).mean():.0f}_B{B}_maxfun{maxfun}"
    evals = float(nfev.sum())
    return {"workload": workload,
            "evals_per_s_per_gpu": evals / (ms * 1e-3), "minimisations_per_s_per_gpu": B / (ms * 1e-3),
            "mean_nfev": float(nfev.mean()), "kernel_ms": ms, "kernel": "k_lds_minimize<8>", "mean_energy": float(np.mean(f)),
            "roofline": counter_roofline("trainable8", workload, "k_lds_minimize<8, false, false>", ms, "hbm", 1, evals)}


def trainable12_aux(tq, B=512, maxfun=1000):
    """BASELINE config 2 at the size the README's table names for TensorRL_trainable/LIH12q_TNbond2 (203 rotations + 37
    CNOTs from |0...0>, every committed rotation a variable; reference environment_qulacs.py:285-328,417-445): fused
    env-step with the workgroup-wide optimiser update on 2 x 208^2 matrices per environment (695 KB, L2 / HBM)."""
    n = 12
    ham = tq.hamiltonian.synthetic_lih12()
    eng = tq.VQEEngine(n)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    rng = np.random.default_rng(1203)
    circs, ths, new = [], [], []
    for b in range(B):
        kind = np.array([0] * 37 + list(rng.integers(1, 4, 203)), np.int32)
        rng.shuffle(kind)
        q0 = rng.integers(0, n, kind.size).astype(np.int32)
        q1 = np.where(kind == 0, (q0 + 1 + rng.integers(0, n - 1, kind.size)) % n, -1).astype(np.int32)
        pidx = np.where(kind > 0, np.cumsum(kind > 0) - 1, -1).astype(np.int32)
        th = rng.uniform(-np.pi, np.pi, 203).astype(np.float32).astype(np.float64)
        last = int(np.nonzero(kind > 0)[0][-1])
        th[pidx[last]] = 0.0
        circs.append(tq.Circuit(kind, q0, q1, pidx, 203)), ths.append(th), new.append(last)
    eng.batch_load(circs, ths)
    eng.batch_set_new_gate(new)
    for _ in range(2):
        eng.batch_run_env_step(1.0, 1e-4, maxfun)
        eng.sync()
    ms = eng.last_kernel_ms()
    _, f, nfev = eng.batch_fetch(want_x=False)
    evals = float(nfev.sum() + B)
    workload = f"lih12_synthetic631_trainable_regime_G240_P202_B{B}_maxfun{maxfun}"
    return {"workload": workload, "evals_per_s_per_gpu": evals / (ms * 1e-3), "env_steps_per_s_per_gpu": B / (ms * 1e-3),
            "mean_nfev": float(nfev.mean()), "kernel_ms": ms, "kernel": "k_lds_minimize<12, true, false>",
            "mean_energy": float(np.mean(f)),
            "roofline": counter_roofline("trainable12", workload, "k_lds_minimize<12, true, false>", ms, "hbm", 4, evals)}


def dm_aux(tq, n, ham, psi0, batch, G, n_circ=4):
    """BASELINE config 5 in the EXACT channel mode (vqe_set_noise_mode(1)): the bench circuits with a depolarising channel
    behind every gate, density matrix of 4^n complex128 (268 MB at 12 qubits), superoperator blocks applied with
    v_mfma_f64_16x16x4_f64 (csrc/vqe_dm.h).  A block sweep reads and writes rho once: algorithmic bytes per evaluation =
    (2 blocks + 1) x 4^n x 16 B; time = device time of the launches (HIP events; the host forms the blocks in between)."""
    B = n_circ
    k = batch["kind"].reshape(-1, G)[:B]; q0 = batch["q0"].reshape(-1, G)[:B]; q1 = batch["q1"].reshape(-1, G)[:B]
    p = batch["pidx"].reshape(-1, G)[:B]
    k2 = np.empty((B, 2 * G), np.int32); a2 = np.empty_like(k2); b2 = np.empty_like(k2); p2 = np.empty_like(k2)
    k2[:, 0::2] = k; k2[:, 1::2] = np.where(k == 0, 5, 4)
    a2[:, 0::2] = q0; a2[:, 1::2] = q0
    b2[:, 0::2] = q1; b2[:, 1::2] = np.where(k == 0, q1, -1)
    p2[:, 0::2] = p; p2[:, 1::2] = -1
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    eng.set_noise(0.01, 0.05, 7)
    eng.set_noise_mode(1)
    par_off = batch["par_off"][:B + 1]
    eng.batch_load_flat(np.arange(B + 1, dtype=np.int64) * 2 * G, k2.ravel(), a2.ravel(), b2.ravel(), p2.ravel(),
                        par_off, batch["theta"][:par_off[-1]])
    t0 = time.perf_counter()
    for _ in range(2):
        eng.batch_run_energy()
        eng.sync()
    wall = (time.perf_counter() - t0) / 2
    ms = eng.last_kernel_ms()
    _, f, _ = eng.batch_fetch(want_x=False)
    blocks = eng.noise_mode_info()["blocks_last_evaluation"]
    byt = B * (2.0 * blocks + 1.0) * (4.0 ** n) * 16.0         # (the last circuit's block count stands for all: same generator)
    gbs = byt / (ms * 1e-3) / 1e9
    workload = f"lih12_synthetic631_fixed_noise_exact_channel_G{G}_B{B}"
    roof = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "traffic": None,
            "kernel": "k_dm_block", "kernel_ms": ms, "algorithmic_bytes": byt,
            "note": "algorithmic bytes (one read + one write of rho per block sweep, one write by the init) / device time of "
                    "the launches of this run"}
    pm, why = load_pmc("dm12", workload)
    if pm is not None and "FETCH_SIZE" in pm.get("per_launch", {}) and "WRITE_SIZE" in pm["per_launch"]:
        c = pm["per_launch"]
        roof["traffic"] = (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0       # per k_dm_block launch
        roof["traffic_per"] = "k_dm_block launch (algorithmic: %.0f)" % (2.0 * (4.0 ** n) * 16.0)
        roof["source"] = pm.get("source")
    else:
        roof["traffic_note"] = why
    return {"workload": workload, "evals_per_s_device": B / (ms * 1e-3), "evals_per_s_wall": B / wall, "blocks_per_evaluation": blocks,
            "kernel_ms": ms, "mean_energy": float(np.mean(f)), "roofline": roof,
            "note": "exact tr(rho H) of the channel the trajectory sampler (noisy12) draws from"}


def mps2qc_stream_aux(tq, dev):
    """The HBM-streaming MPS -> PQC fit (mps2qc_fit_brickwork_stream, beyond the 12 qubits of the LDS-resident kernel):
    18 qubits, one brickwork layer (17 SU(4) gates), 30 Stiefel-Adam steps of one fit.  Per step the kernels sweep the two
    work vectors: G forward applications (read + write psi) and G fused backward sweeps (read + write psi and phi):
    algorithmic bytes per step = G x 96 x 2^n."""
    from tensorrl_qas_amd import dmrg_to_qc as dq
    n, layers, iters = 18, 1, 30
    rng = np.random.default_rng(1818)
    sites, G = dq.brickwork_ansatz(n, layers)
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    target = v / np.linalg.norm(v)
    init = np.array([dq.rand_uni(4, rng) for _ in range(G)])
    opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=True, device_id=dev, stream=True)
    prob = dq.BrickworkOverlap(n, sites, target)
    opt.minimize(prob, init, max_iter=iters, tol=0.0, param_tol=0.0)
    t0 = time.perf_counter()
    opt.minimize(prob, init, max_iter=iters, tol=0.0, param_tol=0.0)
    wall = time.perf_counter() - t0
    steps = int(np.sum(opt.n_iter))
    byt = steps * G * 96.0 * (1 << n)
    ms = opt.kernel_ms
    gbs = byt / (ms * 1e-3) / 1e9
    workload = f"brickwork_fit_stream_{n}q_{layers}layer_G{G}_iters{iters}"
    roof = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "traffic": None,
            "kernel": "k_sf_apply + k_sf_back", "kernel_ms": ms, "algorithmic_bytes": byt,
            "note": "algorithmic bytes G x 96 x 2^n per step / device time reported by the library"}
    pm, why = load_pmc("mps2qc_stream", workload)
    if pm is not None and "FETCH_SIZE" in pm.get("per_launch", {}) and "WRITE_SIZE" in pm["per_launch"]:
        c = pm["per_launch"]
        roof["traffic"] = (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0 * pm.get("launches", 1) / 2.0     # per minimize() call (two calls per run)
        roof["traffic_per"] = "fit of %d steps" % steps
        roof["source"] = pm.get("source")
    else:
        roof["traffic_note"] = why
    return {"workload": workload, "optimiser_steps_per_s_device": steps / (ms * 1e-3), "optimiser_steps_per_s_wall": steps / wall,
            "kernel_ms": ms, "final_loss": float(opt.loss_history[-1]),
            "roofline": roof, "note": "one launch per gate and step (replayed as a hipGraph), Stiefel-Adam update on the host between steps (DESIGN 4.5)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--envs", type=int, default=4096, help="parallel environments per GPU (8 rounds of the 512 "
                    "workgroup slots of the chip: the launch tail costs 4 %% at 2048, 1 %% at 4096)")
    ap.add_argument("--gates", type=int, default=64, help="gates per synthetic circuit")
    ap.add_argument("--maxfun", type=int, default=1000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-heis20", action="store_true")
    ap.add_argument("--no-mps2qc", action="store_true")
    ap.add_argument("--no-sweep", action="store_true", help="skip the G in {8,32,64,110} auxiliary launches")
    ap.add_argument("--no-noisy", action="store_true", help="skip the fixed_noise (config 5) auxiliary launch")
    ap.add_argument("--no-trainable8", action="store_true", help="skip the 8-qubit trainable-regime (config 2) auxiliary launch")
    ap.add_argument("--no-episode8", action="store_true", help="skip the shipped H2O-8q configuration through VecCircuitEnv")
    ap.add_argument("--no-episode", action="store_true", help="skip the LIH12q fixed config through VecCircuitEnv")
    ap.add_argument("--episode", action="store_true", help="(default at N = 1; kept for older command lines)")
    ap.add_argument("--episode-envs", type=int, default=4096)
    ap.add_argument("--episode-steps", type=int, default=110)
    ap.add_argument("--cpu-steps", type=int, default=4)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL); 'gloo' "
                    "only to rehearse the multi-rank code path on a box with fewer GPUs than ranks")
    ap.add_argument("--headline-only", action="store_true", help="only the timed launches of the headline kernel (profiling "
                    "runs: no warm-start / sweep / episode / heis20 / mps2qc / cpu_baseline launches in the trace)")
    ap.add_argument("--selftest-launch", action="store_true", help="CPU rehearsal of the multi-rank launch path (no GPU work)")
    ap.add_argument("--only", default=None, choices=["headline", "noisy12", "trainable8", "trainable12", "dm12", "mps2qc",
                                                      "mps2qc_stream", "heis20"],
                    help="run ONE object of the bench line and print it (tools/pmc_collect.py profiles these commands)")
    ap.add_argument("--no-trainable12", action="store_true")
    ap.add_argument("--no-dm", action="store_true")
    ap.add_argument("--no-mps2qc-stream", action="store_true")
    ap.add_argument("--full", action="store_true", help="also the auxiliary objects of the line (warm start, gate sweep, noisy12, "
                    "trainable8/12, dm12, episode, episode8, heis20, mps2qc, mps2qc_stream, cpu_baseline; each can be left out "
                    "with its --no-* option); without it only the headline launches are timed")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step returned (energy, "
                    "x_opt, nfev per environment) as DIR/<name>.npy in float64")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.only == "headline" or not args.full:
        args.headline_only = True
    if args.headline_only:
        args.no_cpu_baseline = args.no_heis20 = args.no_mps2qc = args.no_sweep = args.no_episode = args.no_noisy = args.no_trainable8 = args.no_episode8 = True
        args.no_trainable12 = args.no_dm = args.no_mps2qc_stream = True

    # ---- launch: under torchrun every process is a rank; started plainly with --gpus N > 1 this process
    # spawns the ranks itself, before anything touches the GPU
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with `python bench.py --gpus N` or "
                         f"`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`")
    if args.selftest_launch:
        return launch_selftest(args, rank, world)

    # Host threads on ONE L3 domain, before anything creates the HIP runtime's helper threads (tensorrl_qas_amd/affinity.py:
    # a loop of ~10 us launches otherwise runs up to 5 x slower on the pool's two-socket hosts, from process to process;
    # VQE_CPU_BIND=0 switches it off).  The BLAS pool of the CPU baseline (--full) is started first, with the full CPU mask.
    global ALL_CPUS
    if hasattr(os, "sched_getaffinity"):
        ALL_CPUS = set(os.sched_getaffinity(0))
        if not args.no_cpu_baseline:
            _ = np.ones((512, 512)) @ np.ones((512, 512))
    import importlib.util
    _spec = importlib.util.spec_from_file_location("vqe_affinity", os.path.join(ROOT, "tensorrl-qas_amd", "affinity.py"))
    _aff = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(_aff)
    cpu_bind = _aff.bind_host_threads(local)

    import torch
    import torch.distributed as dist
    import tensorrl_qas_amd as tq

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the VQE engine has no CPU fallback")
    if args.backend != "nccl":                   # rehearsal: ranks share the visible GPUs
        local = local % torch.cuda.device_count()
    elif world > torch.cuda.device_count():
        raise SystemExit(f"--gpus {world} but only {torch.cuda.device_count()} GPUs are visible")
    torch.cuda.set_device(local)
    torch.cuda.set_stream(torch.cuda.Stream())   # one explicit stream for the engine, copies and RCCL
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local}"))
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    ranks_seen = dist.get_world_size() if world > 1 else 1

    n, B, G = N_QUBITS, args.envs, args.gates
    ham = tq.hamiltonian.synthetic_lih12()
    psi0 = tq.hamiltonian.brickwork_state(n, 12)
    eng = tq.VQEEngine(n, local)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    batch = make_batch(tq, n, B, G, 1000 + rank)
    eng.batch_load_flat(batch["gate_off"], batch["kind"], batch["q0"], batch["q1"], batch["pidx"],
                        batch["par_off"], batch["theta"])
    eng.batch_set_new_gate(batch["new_gate"])

    if args.only and args.only != "headline":      # one object of the line (profiling commands)
        if args.only == "noisy12":
            obj = noisy_aux(tq, n, ham, psi0, batch, B, G, args.maxfun)
        elif args.only == "trainable8":
            obj = trainable8_aux(tq)
        elif args.only == "trainable12":
            obj = trainable12_aux(tq)
        elif args.only == "dm12":
            obj = dm_aux(tq, n, ham, psi0, batch, G)
        elif args.only == "mps2qc":
            obj = mps2qc_aux(tq, local, False)
        elif args.only == "mps2qc_stream":
            obj = mps2qc_stream_aux(tq, local)
        else:
            obj = heis20_aux(tq, torch, dist, rank, world, local, max(2, args.steps))
        if rank == 0:
            print(json.dumps({"only": args.only, **obj}), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    def step():
        eng.batch_run_env_step(1.0, 1e-4, args.maxfun)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tt = torch.tensor([dt], dtype=torch.float64, device=f"cuda:{local}")
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt = float(tt.item())
    # kernel duration (HIP events on the launch stream) of the last step, and its work
    k_ms = eng.last_kernel_ms()
    x_last, f, nfev = eng.batch_fetch(want_x=args.dump_outputs is not None)
    if args.dump_outputs is not None:
        dump_outputs(args.dump_outputs, {"energy": f, "x_opt": x_last, "nfev": nfev}, rank, world)
    evals_per_launch = int(nfev.sum()) + B          # + the final post-action evaluation
    T, Tx = ham.n_terms, ham.n_xgroups
    bytes_per_eval = (2 ** n) * 16 * (2 * (G - 1) + T)          # 2^n*16*(2G+T)
    bytes_per_eval_grouped = (2 ** n) * 16 * (2 * (G - 1) + Tx)
    stats = torch.tensor([float(nfev.sum()), float(B)], dtype=torch.float64, device=f"cuda:{local}")
    if world > 1:
        dist.all_reduce(stats)
    mean_nfev = float(stats[0].item() / stats[1].item())

    # auxiliary: the same batch warm-started from its own optimum (what an RL episode does:
    # x0 of a step is the previous step's optimum), one fused launch
    warm = None
    if not args.headline_only:
        x_opt, _, _ = eng.batch_fetch()
        eng.batch_load_flat(batch["gate_off"], batch["kind"], batch["q0"], batch["q1"], batch["pidx"],
                            batch["par_off"], x_opt)
        eng.batch_set_new_gate(batch["new_gate"])
        eng.batch_run_env_step(1.0, 1e-4, args.maxfun)
        torch.cuda.synchronize()
        warm_ms = eng.last_kernel_ms()
        _, _, nfev_w = eng.batch_fetch(want_x=False)
        warm = {"env_steps_per_s_per_gpu": B / (warm_ms * 1e-3), "mean_nfev": float(nfev_w.mean()),
                "note": "same circuits, x0 = optimum of the previous step (float32), kernel time only"}
    sweep = None if args.no_sweep else g_sweep(tq, eng, n, B, args.maxfun, rank)
    noisy = None if (args.no_noisy or rank != 0) else noisy_aux(tq, n, ham, psi0, batch, B, G, args.maxfun)
    train8 = None if (args.no_trainable8 or rank != 0) else trainable8_aux(tq)
    train12 = None if (args.no_trainable12 or rank != 0) else trainable12_aux(tq)
    dm12 = None if (args.no_dm or rank != 0) else dm_aux(tq, n, ham, psi0, batch, G)

    episode = None
    if not args.no_episode and rank == 0 and world == 1:
        episode = episode_aux(tq, torch, local, args.episode_envs, args.episode_steps)
    episode8 = None
    if not args.no_episode8 and rank == 0 and world == 1:
        episode8 = episode8_aux(tq, torch, local)
    if world > 1:
        dist.barrier()

    heis = None
    if not args.no_heis20:
        heis = heis20_aux(tq, torch, dist, rank, world, local, max(2, args.steps))

    if rank == 0:
        workload = f"lih12_synthetic631_fixed_noiseless_G{G}_B{B}_per_gpu"
        roof = counter_roofline("headline", workload, "k_lds_minimize<12, false, false>", k_ms, "fp64_valu", 4, evals_per_launch)
        roof.setdefault("note", "executed FP64 vector flops (2 FMA + MUL + ADD wave instructions x 64 lanes) of one launch / kernel "
                        "duration of this run; the state never leaves VGPRs / LDS, so neither HBM nor MFMA binds - the FP64 vector "
                        "pipe peaks at the same 78.6 TFLOP/s as the FP64 matrix pipe on MI355X.  The energy step skips the exact "
                        "zeros of the sign-sum tables (unit path, round 3): fewer flops are EXECUTED per evaluation than in "
                        "rounds 1-2 (dense_equivalent below is the old kernel's flop count over this run's time)")
        if roof.get("achieved") is not None:
            # the flops the round-2 kernel executed for the same workload (profiles/r02g_pmc_sq.txt: 7.254e12 per launch of
            # 4 100 061 evaluations), at this run's rate: comparable with the fractions of rounds 1 and 2
            dense = 7.254e12 / 4100061.0 * evals_per_launch
            roof["dense_equivalent"] = {"flop_per_launch": dense, "achieved": dense / (k_ms * 1e-3) / 1e12,
                                        "frac": dense / (k_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                                        "note": "NOT executed work: the round-2 kernel's flops for these evaluations / this run's time"}
        roof.update({"evaluations_per_launch": evals_per_launch,
                     "algorithmic": {"bytes_per_evaluation": bytes_per_eval, "bytes_per_evaluation_xgrouped": bytes_per_eval_grouped,
                                     "GBs_if_streamed_from_hbm": evals_per_launch * bytes_per_eval / (k_ms * 1e-3) / 1e9,
                                     "note": "SURVEY 8d figure 2^n*16*(2G+T) x evaluations / kernel time: what a kernel that "
                                             "streamed the state through HBM for every gate and term would have to move; "
                                             "informational only - this kernel keeps the state in VGPRs / LDS"}})
        out = {
            "metric": "VQE env-steps/sec", "value": world * B * args.steps / dt, "unit": "env-steps/s",
            "n_gpus": world, "ranks_seen": ranks_seen, "backend": args.backend if world > 1 else None,
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": workload,
                       "n_qubits": n, "pauli_terms": T, "x_groups": Tx, "gates": G, "envs_per_gpu": B,
                       "cobyla": {"rhobeg": 1.0, "rhoend": 1e-4, "maxfun": args.maxfun},
                       "mean_nfev": mean_nfev, "parallelism": f"env-replicas x{world}",
                       "host_threads": ("%d logical CPUs of one L3 domain, first %d (tensorrl_qas_amd.bind_host_threads; the CPU baseline "
                                        "runs on all %d)" % (len(cpu_bind), min(cpu_bind), len(ALL_CPUS or ()))) if cpu_bind else "unbound"},
            "evals_per_s": world * evals_per_launch / (k_ms * 1e-3),
            "energy_checksum": float(np.sum(f)),
            "roofline": roof,
        }
        if warm is not None:
            out["warm_start"] = warm
        if sweep is not None:
            out["gate_sweep"] = sweep
        if noisy is not None:
            out["noisy12"] = noisy
        if train8 is not None:
            out["trainable8"] = train8
        if train12 is not None:
            out["trainable12"] = train12
        if dm12 is not None:
            out["dm12"] = dm12
        if episode is not None:
            out["episode"] = episode
        if episode8 is not None:
            out["episode8"] = episode8
        if heis is not None:
            out["heis20"] = heis
        if not args.no_mps2qc:
            out["mps2qc"] = mps2qc_aux(tq, local, not args.no_cpu_baseline and world == 1)
        if not args.no_mps2qc_stream:
            out["mps2qc_stream"] = mps2qc_stream_aux(tq, local)
        if not args.no_cpu_baseline and world == 1:      # timed at N = 1 only
            out["cpu_baseline"] = cpu_baseline(tq, ham, psi0, batch, G, args.cpu_steps, args.maxfun)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
