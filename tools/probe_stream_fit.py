#!/usr/bin/env python3
"""The streaming MPS -> PQC fit with the Stiefel-Adam update on the host (mps2qc_fit_brickwork_stream) beside the resident
streaming fit (mps2qc_fit_brickwork_resident, update on the device), alternating in ONE process: one warm-up round, then 5
rounds, every variant once per round; median and spread (min .. max) of the library's device time (HIP events around the
whole loop) and of the wall time of the Python call.

  bench     the mps2qc_stream workload of bench.py: 18 qubits, 1 layer (17 gates), 30 steps, one fit, random target
  heis20    the workload of tools/make_heis20_init.py: the 20-qubit Heisenberg ground state (device Lanczos), 1 layer
            (19 gates), 600 steps x 2 restarts, optimiser 3e-2; the device update with check_every 1, 8 and 64.  Wall
            time here is the chain from "ground state on the device" to "gates on the host": the host update first
            copies the state to the host and bit-reverses it in numpy (the host hop), the device update reads the tensor.

    python3 tools/probe_stream_fit.py [out.json]        (profiles/stream_fit_resident.json by default; needs a GPU)
    PROBE_ONLY=bench PROBE_REPS=1 ...                   one workload, fewer rounds (what the kernel-trace run uses)

The table it prints is in DESIGN 4.15."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensorrl_qas_amd as tq  # noqa: E402
from tensorrl_qas_amd import dmrg_to_qc as dq  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_fit_resident.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
only = os.environ.get("PROBE_ONLY", "")
reps = int(os.environ.get("PROBE_REPS", "5"))
variants_env = os.environ.get("PROBE_VARIANTS", "")


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def measure(variants):
    """variants: name -> callable returning (device_ms, result); one warm-up round, then `reps` rounds"""
    if variants_env:
        variants = {k: f for k, f in variants.items() if k in variants_env.split(",")}
    dev = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    last = {}
    for rnd in range(reps + 1):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            ms, res = fn()
            w = (time.perf_counter() - t0) * 1e3
            if rnd:
                dev[name].append(ms), wall[name].append(w)
            last[name] = res
    return dev, wall, last


rows = []

if only in ("", "bench"):
    n, layers, iters = 18, 1, 30
    rng = np.random.default_rng(1818)
    sites, G = dq.brickwork_ansatz(n, layers)
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    target = v / np.linalg.norm(v)
    init = np.array([dq.rand_uni(4, rng) for _ in range(G)])
    prob = dq.BrickworkOverlap(n, sites, target)

    def run_bench(update, check_every=8):
        opt = dq.StiefelAdam(3e-3, 0.9, 0.999, 1e-8, jit_frozen=True, stream=True, update=update, check_every=check_every)
        opt.minimize(prob, init, max_iter=iters, tol=0.0, param_tol=0.0)
        return opt.kernel_ms, opt

    dev, wall, last = measure({"host": lambda: run_bench("host"), "device_ce8": lambda: run_bench("device", 8),
                               "device_ce30": lambda: run_bench("device", 30)})
    for k in dev:
        row = {"workload": f"bench mps2qc_stream: {n} qubits, G = {G}, {iters} steps, 1 fit", "variant": k,
               "launches_per_step": (3 * G + 5) if k == "host" else (2 * G + 5), "copies_per_step": 3 if k == "host" else 0,
               "steps_enqueued": last[k].steps_enqueued, "device_ms": stats(dev[k]), "wall_ms": stats(wall[k]),
               "final_loss": float(last[k].loss_history[-1]),
               "max_history_difference_to_host": float(np.max(np.abs(np.array(last[k].loss_history) - np.array(last["host"].loss_history))))
               if "host" in last else None}
        rows.append(row)
        print(json.dumps(row), flush=True)

if only in ("", "heis20"):
    import torch
    n, layers, iters, restarts = int(os.environ.get("HEIS_N", "20")), 1, 600, 2
    ham, _ = tq.hamiltonian.heisenberg(n)
    e0, vec = tq.hamiltonian.ground_state_device(ham, return_tensor=True)
    sites, G = dq.brickwork_ansatz(n, layers)
    rev = dq.stiefel_opt.bit_reversed(n)
    opts = {"max_iter": iters, "tol": 1e-10, "param_tol": 1e-9}
    ansatz = {"structure": "brickwork", "num_layers": layers}

    def run_hop():
        opt = dq.StiefelAdam(3e-2, 0.9, 0.999, 1e-8, update="host")
        psi = vec.cpu().numpy()
        dq.mps_to_qc(psi[rev], ansatz, {"method": opt, **opts}, n_restarts=restarts, rng=np.random.default_rng(20))
        return opt.kernel_ms, opt

    def run_resident(check_every):
        opt = dq.StiefelAdam(3e-2, 0.9, 0.999, 1e-8, update="device", check_every=check_every)
        dq.mps_to_qc(vec, ansatz, {"method": opt, **opts}, n_restarts=restarts, rng=np.random.default_rng(20), target_order="little_endian")
        return opt.kernel_ms, opt

    dev, wall, last = measure({"host": run_hop, "device_ce1": lambda: run_resident(1), "device_ce8": lambda: run_resident(8),
                               "device_ce64": lambda: run_resident(64)})
    for k in dev:
        row = {"workload": f"heis{n}: {n} qubits, G = {G}, {iters} steps x {restarts} restarts", "variant": k,
               "launches_per_step": (3 * G + 5) if k == "host" else (2 * G + 5), "copies_per_step": 3 if k == "host" else 0,
               "steps_enqueued": last[k].steps_enqueued, "n_iter": [int(x) for x in last[k].n_iter],
               "fit_device_ms": stats(dev[k]), "chain_wall_ms_ground_state_on_device_to_gates_on_host": stats(wall[k]),
               "host_hop": k == "host", "best_val": [float(x) for x in last[k].best_val]}
        rows.append(row)
        print(json.dumps(row), flush=True)

json.dump({"script": "tools/probe_stream_fit.py", "rounds": f"1 warm-up + {reps}, variants alternating within a round",
           "device_ms": "HIP events around the whole optimisation loop, as the library reports it (total_ms)",
           "rows": rows}, open(out, "w"), indent=1)
print("| workload | variant | launches / step | copies / step | device ms (median, min .. max) | wall ms (median, min .. max) |\n|---|---|---|---|---|---|")
for r in rows:
    d = r.get("device_ms") or r.get("fit_device_ms")
    w = r.get("wall_ms") or r.get("chain_wall_ms_ground_state_on_device_to_gates_on_host")
    print(f"| {r['workload']} | {r['variant']} | {r['launches_per_step']} | {r['copies_per_step']} | "
          f"{d['median']:.2f} ({d['min']:.2f} .. {d['max']:.2f}) | {w['median']:.2f} ({w['min']:.2f} .. {w['max']:.2f}) |")
