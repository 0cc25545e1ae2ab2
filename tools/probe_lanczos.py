#!/usr/bin/env python3
"""Device Lanczos (VQEEngine.lanczos, csrc/vqe_lanczos.h) beside the host Lanczos of hamiltonian._lanczos (scipy eigsh on
a numpy LinearOperator) in one session: the lowest eigenpair of the Heisenberg chains of n = 12, 16, 20 qubits and of the
synthetic 12-qubit LiH.  Per problem: the device time (vqe_last_kernel_ms, median of 5 after 2 warm-ups), the number of H
applications, the wall time of the host path and the difference of the two eigenvalues.

    python3 tools/probe_lanczos.py [out.json]        (profiles/lanczos.json by default; needs a GPU)

    python3 tools/probe_lanczos.py --multi [out.json]   (profiles/lanczos_multi.json by default)

--multi: several eigenpairs (VQEEngine.lanczos_multi: thick restart, locking) beside vqe_lanczos of the same build in the
same session, on the same problems: device ms (median of 3 after 1 warm-up) and H applications for k = 1 and k = 4 at the
library's defaults, and the k = 1 figures of both entry points at max_basis 4, 8 and 128 (max_matvec 5000).

The tables it prints are in DESIGN 4.14."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensorrl_qas_amd as tq  # noqa: E402

multi = "--multi" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != "--multi"]
out = args[0] if args else os.path.join(ROOT, "profiles", "lanczos_multi.json" if multi else "lanczos.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
problems = [(f"heisenberg_{n}q", tq.hamiltonian.heisenberg(n)[0]) for n in (12, 16, 20)]
problems.append(("synthetic_LiH12", tq.hamiltonian.synthetic_lih12()))


def timed(eng, call, reps=4):
    ms = []
    for _ in range(reps):
        res = call()
        ms.append(eng.last_kernel_ms())
    return res, statistics.median(ms[1:])


if multi:
    rows = []
    for name, ham in problems:
        eng = tq.VQEEngine(ham.n)
        eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
        for basis in (128, 8, 4):
            (val, _, info), ms = timed(eng, lambda: eng.lanczos("min", want_vector=False, max_basis=basis, max_matvec=5000))
            rows.append({"problem": name, "entry": "vqe_lanczos", "k": 1, "max_basis": basis, "device_ms": ms, "matvecs": info["matvecs"],
                         "restarts": info["restarts"], "status": info["status_name"], "residual": info["residual"], "values": [val]})
            print(json.dumps(rows[-1]), flush=True)
            for k in ((1, 4) if basis == 128 else (1,)):
                (vals, _, info), ms = timed(eng, lambda: eng.lanczos_multi(k, "min", want_vectors=False, max_basis=basis, max_matvec=5000))
                rows.append({"problem": name, "entry": "vqe_lanczos_multi", "k": k, "max_basis": basis, "device_ms": ms,
                             "matvecs": info["matvecs"], "restarts": info["restarts"], "status": info["status_name"],
                             "residual": info["residual"], "pairs": info["pairs"], "values": [float(v) for v in vals]})
                print(json.dumps(rows[-1]), flush=True)
        eng.close()
    json.dump({"script": "tools/probe_lanczos.py --multi", "options": "tol 1e-10, check_every 8, seed 1, keep 0, max_matvec 5000",
               "rows": rows}, open(out, "w"), indent=1)
    print("| problem | entry | k | max_basis | H applications | restarts | device ms | status |\n|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['problem']} | {r['entry']} | {r['k']} | {r['max_basis']} | {r['matvecs']} | {r['restarts']} | {r['device_ms']:.2f} | {r['status']} |")
    sys.exit(0)

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
