"""Throughput of the Pauli channel tables of the mode 0 sampler (vqe_set_noise_pauli) -> profiles/noise_pauli.json.

At 12 qubits (LDS-resident path, fused energy kernel) and at 20 qubits (streaming path), on the same circuits and in the
same session: evaluations/s of batch_run_energy
  * with a biased (dephasing-heavy) table in both slots,
  * with the depolarising sampler at the same total probabilities,
  * on the quantum-jump path with T = 1 and the same channel as a Kraus override (channels.pauli_channel).

    python tools/probe_noise_pauli.py [out.json]

The parent process never opens the GPU: every step runs in a child of its own under `timeout`, and the first step that
fails ends the probe."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT = {12: 240, 20: 420}
BATCH = {12: 4096, 20: 8}
GATES, REPS = 32, 5


def step(n, out_path):
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import numpy as np
    import tensorrl_qas_amd as tq
    from helpers import random_gates, random_hamiltonian, random_state, with_noise_gates
    rng = np.random.default_rng(1200 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 40, rng, real=False)
    w1 = np.array([0.002, 0.002, 0.026])
    w2 = np.full(15, 0.001)
    w2[[3 - 1, 12 - 1, 15 - 1]] = 0.016
    p1, p2 = float(np.cumsum(w1)[-1]), float(np.cumsum(w2)[-1])
    pool = []
    for _ in range(64):
        kind, q0, q1, pidx, th = random_gates(n, GATES, rng, p_cnot=0.3)
        pool.append((with_noise_gates(kind, q0, q1, pidx), th))
    B = BATCH[n]
    batch = [pool[i % 64] for i in range(B)]

    def engine(p=(0.0, 0.0)):
        e = tq.VQEEngine(n)
        e.set_init_state(psi0)
        e.set_hamiltonian(*ham)
        e.set_noise(p[0], p[1], 7)
        return e

    def timed(eng, reps=REPS):
        eng.batch_load([tq.Circuit(*g, th.size) for g, th in batch], [th for _, th in batch])
        eng.batch_run_energy()                      # warm-up (tables, plans, allocations)
        eng.sync()
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.batch_run_energy()
            eng.sync()
            best = min(best, time.perf_counter() - t0)
        return best

    table = engine()
    table.set_noise_pauli(w1, w2)
    dt_table = timed(table)
    info = table.device_info()
    dt_depol = timed(engine((p1, p2)))
    jump = engine()
    jump.set_noise_kraus(tq.channels.pauli_channel(w1), tq.channels.pauli_channel(w2))
    jump.set_kraus_traj(1)
    if n >= 14:
        jump.set_stream_kraus_traj(-1)
    dt_jump = timed(jump, reps=2 if n >= 14 else REPS)
    row = {"n": n, "batch": B, "p1": p1, "p2": p2,
           "table_seconds": dt_table, "table_evaluations_per_s": B / dt_table,
           "depolarising_seconds": dt_depol, "depolarising_evaluations_per_s": B / dt_depol,
           "quantum_jump_T1_seconds": dt_jump, "quantum_jump_T1_evaluations_per_s": B / dt_jump}
    print(row, flush=True)
    json.dump({"device": {k: int(v) for k, v in info.items()}, "row": row}, open(out_path, "w"), indent=1)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "noise_pauli.json")
    merged = {"gates_per_circuit": 2 * GATES, "tables": "w1 = (0.002, 0.002, 0.026); w2 = 0.016 at Z., .Z, ZZ and 0.001 elsewhere",
              "timing": f"best of {REPS} batch_run_energy + sync (quantum jumps at 20 qubits: best of 2), one warm-up", "steps": []}
    for n in (12, 20):
        part = f"{out}.n{n}.part"
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT[n]), sys.executable, os.path.abspath(__file__), "--step", str(n), part]).returncode
        if rc != 0:
            print(f"step n={n} ended with status {rc}: the probe stops here", file=sys.stderr)
            return rc
        merged["steps"].append(json.load(open(part)))
        os.remove(part)
    json.dump(merged, open(out, "w"), indent=1)
    print(f"wrote {out}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        step(int(sys.argv[2]), sys.argv[3])
    else:
        sys.exit(main())
