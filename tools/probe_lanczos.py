#!/usr/bin/env python3
"""Device Lanczos (VQEEngine.lanczos, csrc/vqe_lanczos.h) beside the host Lanczos of hamiltonian._lanczos (scipy eigsh on
a numpy LinearOperator) in one session: the lowest eigenpair of the Heisenberg chains of n = 12, 16, 20 qubits and of the
synthetic 12-qubit LiH.  Per problem: the device time (vqe_last_kernel_ms, median of 5 after 2 warm-ups), the number of H
applications, the wall time of the host path and the difference of the two eigenvalues.

    python3 tools/probe_lanczos.py [out.json]        (profiles/lanczos.json by default; needs a GPU)

The table it prints is in DESIGN 4.14."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensorrl_qas_amd as tq  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lanczos.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
problems = [(f"heisenberg_{n}q", tq.hamiltonian.heisenberg(n)[0]) for n in (12, 16, 20)]
problems.append(("synthetic_LiH12", tq.hamiltonian.synthetic_lih12()))
rows = []
for name, ham in problems:
    eng = tq.VQEEngine(ham.n)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    ms, wall = [], []
    for rep in range(7):
        t0 = time.perf_counter()
        val, _, info = eng.lanczos("min", want_vector=False)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(eng.last_kernel_ms())
    t0 = time.perf_counter()
    e_host, _ = tq.hamiltonian.ground_state(ham)
    host_s = time.perf_counter() - t0
    row = {"problem": name, "n_qubits": ham.n, "terms": ham.n_terms, "x_groups": ham.n_xgroups,
           "device_ms": statistics.median(ms[2:]), "device_call_wall_ms": statistics.median(wall[2:]),
           "matvecs": info["matvecs"], "restarts": info["restarts"], "status": info["status_name"], "residual": info["residual"],
           "host_lanczos_s": host_s, "eigenvalue_device": val, "eigenvalue_host": e_host, "difference": val - e_host}
    rows.append(row)
    print(json.dumps(row), flush=True)
    eng.close()
json.dump({"script": "tools/probe_lanczos.py", "options": "library defaults (basis 128, tol 1e-10, check_every 8, seed 1)",
           "rows": rows}, open(out, "w"), indent=1)
print("| problem | H applications | device ms | host s | eigenvalue difference |\n|---|---|---|---|---|")
for r in rows:
    print(f"| {r['problem']} | {r['matvecs']} | {r['device_ms']:.2f} | {r['host_lanczos_s']:.2f} | {r['difference']:.1e} |")
