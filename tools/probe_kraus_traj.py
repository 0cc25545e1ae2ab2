"""Throughput of the quantum-jump trajectories of a Kraus channel (vqe_set_kraus_traj) -> profiles/kraus_traj.json.

At 8 and 12 qubits, B = 64 and the CU-filling batch of device_info(), T in {1, 16, 128}: trajectories/s and
evaluations/s of batch_run_energy; on the same circuits and in the same session the batched exact channel
(set_noise_mode(1) + set_dm_batched(-1), B = 64) and the depolarising Pauli-trajectory path (the ceiling: one trajectory
per evaluation in the fused energy kernel); and the T at which T trajectories cost one exact evaluation.

    python tools/probe_kraus_traj.py [out.json]

The parent process never opens the GPU: every step runs in a child of its own under `timeout`, and the first step that
fails ends the probe."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT = {8: 120, 12: 240}
GATES, REPS = 24, 5


def step(n, out_path):
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import numpy as np
    import tensorrl_qas_amd as tq
    import qj_cases as qc
    from helpers import random_hamiltonian, random_state
    rng = np.random.default_rng(900 + n)
    psi0 = random_state(n, rng)
    ham = random_hamiltonian(n, 40, rng, real=False)
    K1, K2 = qc.combo("damping+product")

    def engine():
        e = tq.VQEEngine(n)
        e.set_init_state(psi0)
        e.set_hamiltonian(*ham)
        e.set_noise(0.01, 0.05, 7)
        return e

    def timed(eng, reps=REPS):
        eng.batch_run_energy()                      # warm-up (tables, plans, allocations)
        eng.sync()
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.batch_run_energy()
            eng.sync()
            best = min(best, time.perf_counter() - t0)
        return best

    probe = engine()
    info = probe.device_info()
    rows = []
    cu_fill = None
    for B in (64, None):
        circuits = [qc.noisy_su4(n, GATES, rng) for _ in range(64)]
        traj = engine()
        traj.set_noise_kraus(K1, K2)
        for T in (1, 16, 128):
            traj.set_kraus_traj(T)
            if B is None:                           # what the device holds of this kernel: CUs x workgroups per CU
                if cu_fill is None:
                    traj.batch_load([tq.Circuit(*c[:4], c[4].size) for c in circuits], [c[4] for c in circuits])
                    traj.batch_run_energy()
                    cu_fill = int(traj.device_info()["cu_count"] * max(1, traj.device_info()["wg_per_cu"]))
                nb = cu_fill
            else:
                nb = B
            batch = [circuits[i % 64] for i in range(nb)]
            traj.batch_load([tq.Circuit(*c[:4], c[4].size) for c in batch], [c[4] for c in batch])
            dt = timed(traj)
            rows.append({"n": n, "batch": nb, "cu_filling": B is None, "T": T, "seconds": dt, "trajectories_per_s": nb * T / dt,
                         "evaluations_per_s": nb / dt, "workgroups": traj.kraus_traj_info()["workgroups"]})
            print(rows[-1], flush=True)
        if B == 64:
            batch = circuits
            exact = engine()
            exact.set_noise_mode(1)
            exact.set_dm_batched(-1)
            exact.set_dm_rot2(True)
            exact.set_noise_kraus(K1, K2)
            exact.batch_load([tq.Circuit(*c[:4], c[4].size) for c in batch], [c[4] for c in batch])
            dt_exact = timed(exact, reps=2)
            pauli = engine()
            pauli.batch_load([tq.Circuit(*c[:4], c[4].size) for c in batch], [c[4] for c in batch])
            dt_pauli = timed(pauli)
            per_traj = [r["seconds"] / (r["batch"] * r["T"]) for r in rows if r["batch"] == 64 and r["T"] == 128][0]
            rows.append({"n": n, "batch": 64, "exact_seconds": dt_exact, "exact_evaluations_per_s": 64 / dt_exact,
                         "exact_resident": exact.dm_batch_info()["resident"], "pauli_seconds": dt_pauli,
                         "pauli_trajectories_per_s": 64 / dt_pauli, "break_even_T": (dt_exact / 64) / per_traj})
            print(rows[-1], flush=True)
    json.dump({"device": {k: int(v) for k, v in info.items()}, "rows": rows}, open(out_path, "w"), indent=1)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kraus_traj.json")
    merged = {"gates_per_circuit": 2 * GATES, "channels": "amplitude_damping(0.3) / tensor(amplitude_damping(0.25), dephasing(0.2))",
              "timing": f"best of {REPS} batch_run_energy + sync (exact: best of 2), one warm-up", "steps": []}
    for n in (8, 12):
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
