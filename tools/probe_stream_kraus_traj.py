"""Throughput of the quantum-jump trajectories on the streaming path (vqe_set_stream_kraus_traj, n >= 14)
-> profiles/stream_kraus_traj.json.

At 14, 16 and 20 qubits, circuits of 64 gates with a channel behind every gate, T in {1, 16}, and B chosen so that the
B T resident states fill the device (8 workgroups of a state sweep per CU, at least one circuit): evaluations/s and
ms per evaluation of batch_run_energy, and the sweeps per evaluation the handle reports.  On the same handle, with the
override removed, the same B T circuits under depolarising Pauli trajectories (the existing streaming path: one state
per circuit, the T = 1 equivalent).  No threshold is asserted: the figures are what this probe exists to find out.

    python tools/probe_stream_kraus_traj.py [out.json]

The parent process never opens the GPU: every size runs in a child of its own under `timeout`, and the first step that
fails ends the probe.  The result is printed as one JSON line and written to the file."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (14, 16, 20)
STEP_TIMEOUT = 300
GATES, REPS, WG_PER_CU = 64, 3, 8


def step(n, out_path):
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import numpy as np
    import tensorrl_qas_amd as tq
    import qj_cases as qc
    from helpers import random_hamiltonian, random_state
    rng = np.random.default_rng(1400 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 40, rng, real=False)
    K1, K2 = qc.combo("damping+product")
    eng = tq.VQEEngine(n)
    eng.set_init_state(psi0)
    eng.set_hamiltonian(*ham)
    eng.set_noise(0.01, 0.05, 7)
    info = eng.device_info()
    sweep_blocks = (1 << n) // 2 // 2048                 # workgroups of one state's sweep (kSqGroups of csrc/vqe_stream_qjump.h)
    states = max(16, -(-WG_PER_CU * int(info["cu_count"]) // sweep_blocks))
    states = -(-states // 16) * 16
    circuits = [qc.noisy_su4(n, GATES, rng) for _ in range(8)]

    def load(count):
        batch = [circuits[i % len(circuits)] for i in range(count)]
        eng.batch_load([tq.Circuit(*c[:4], c[4].size) for c in batch], [c[4] for c in batch])

    def timed():
        eng.batch_run_energy()                           # warm-up (tables, plans, allocations)
        eng.sync()
        best = float("inf")
        for _ in range(REPS):
            t0 = time.perf_counter()
            eng.batch_run_energy()
            eng.sync()
            best = min(best, time.perf_counter() - t0)
        return best

    rows = []
    eng.set_noise_kraus(K1, K2)
    eng.set_stream_kraus_traj(-1)
    for T in (1, 16):
        B = states // T
        eng.set_kraus_traj(T)
        load(B)
        dt = timed()
        s = eng.stream_kraus_traj_info()
        rows.append({"n": n, "batch": B, "T": T, "states": B * T, "ms_per_evaluation": 1e3 * dt / B, "evaluations_per_s": B / dt,
                     "trajectories_per_s": B * T / dt, "seconds": dt, "resident": s["resident"], "chunks": s["chunks"],
                     "rounds": s["rounds"], "sweeps_per_evaluation": s["sweeps"] * s["chunks"], "jumps": eng.kraus_traj_info()["jumps"]})
        print(rows[-1], flush=True)
    eng.set_noise_kraus(None, None)                      # the same handle on depolarising Pauli trajectories
    eng.set_kraus_traj(0)
    load(states)
    dt = timed()
    rows.append({"n": n, "batch": states, "pauli_ms_per_evaluation": 1e3 * dt / states, "pauli_evaluations_per_s": states / dt,
                 "pauli_seconds": dt, "kraus_T1_over_pauli": rows[0]["seconds"] / dt})
    print(rows[-1], flush=True)
    json.dump({"device": {k: int(v) for k, v in info.items()}, "rows": rows}, open(out_path, "w"))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_kraus_traj.json")
    merged = {"command": "python tools/probe_stream_kraus_traj.py", "gates_per_circuit": 2 * GATES,
              "channels": "amplitude_damping(0.3) / tensor(amplitude_damping(0.25), dephasing(0.2))",
              "timing": f"best of {REPS} batch_run_energy + sync, one warm-up", "steps": []}
    for n in SIZES:
        part = f"{out}.n{n}.part"
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(n), part]).returncode
        if rc != 0:
            print(f"step n={n} ended with status {rc}: the probe stops here", file=sys.stderr)
            return rc
        merged["steps"].append(json.load(open(part)))
        os.remove(part)
    line = json.dumps(merged)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        step(int(sys.argv[2]), sys.argv[3])
    else:
        sys.exit(main())
