"""Device Adam-SPSA env-step (vqe_batch_run_env_step_spsa) against the device COBYLA env-step (vqe_batch_run_env_step) in
one process, at the same evaluation budget (COBYLA maxfun = 2 K, Adam-SPSA maxiter = K), on three shapes:
  fixed     12 qubits /  32 variables / 4096 environments (the headline workload's shape, synthetic LiH-12q),
  trainable  8 qubits / 129 variables / 4096 environments (H2O-8q),
  trainable 12 qubits / 202 variables /  512 environments (synthetic LiH-12q).
The new gate of every environment is its last gate.  Kernel times by HIP events on the handle's stream: two warm-up
launches, then `--reps` timed ones (default 7); reported are the median, the smallest and the largest, the evaluations
per second at the median (evaluations = sum of nfev, which COBYLA may end below its budget), and the mean final energy.

Then, with depolarising noise (p1 = 0.01, p2 = 0.05) on 64 noisy 8-qubit circuits: the mean exact-channel energy
(vqe_set_noise_mode 1 on a second handle) at the point each optimiser returns.

Writes profiles/spsa.json and prints the table of DESIGN 4.22.
usage: probe_spsa.py [--scale S] [--reps R] [--budget 2K]   (--scale multiplies every batch size, for quick runs)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tensorrl_qas_amd as tq  # noqa: E402
from probe_grad import circuits  # noqa: E402


def timed(eng, run, reps):
    for _ in range(2):
        run()
    eng.sync()
    ms = []
    for _ in range(reps):
        run()
        eng.sync()
        ms.append(eng.last_kernel_ms())
    return ms


def arg(name, default, cast):
    a = sys.argv[1:]
    return cast(a[a.index(name) + 1]) if name in a else default


def with_noise_gates(c):
    kind, q0, q1, pidx = [], [], [], []
    for k, a, b, p in zip(c.kind, c.q0, c.q1, c.pidx):
        kind += [int(k), 5 if k == 0 else 4]
        q0 += [int(a), int(a)]
        q1 += [int(b), int(b) if k == 0 else -1]
        pidx += [int(p), -1]
    return tq.Circuit(kind, q0, q1, pidx, c.n_params)


def main():
    scale, reps, budget = arg("--scale", 1.0, float), arg("--reps", 7, int), arg("--budget", 200, int)
    K = budget // 2
    d = np.load(os.path.join(ROOT, "tests", "golden", "ham_H2O_8q.npz"))
    xs, zs = tq.hamiltonian.masks_from_strings([str(s) for s in d["paulis"]], 8)
    h2o = (xs, zs, np.asarray(d["weights"], float))
    lih = tq.hamiltonian.synthetic_lih12()
    lih = (lih.xmask, lih.zmask, lih.coeff)
    shapes = [("fixed 12q P=32", 12, 32, 12, 4096, lih), ("trainable 8q P=129", 8, 129, 21, 4096, h2o),
              ("trainable 12q P=202", 12, 202, 37, 512, lih)]
    rng = np.random.default_rng(2026)
    out = {"budget": budget, "maxiter": K, "reps": reps, "shapes": [], "noise": None}
    rows = []
    for name, n, P, nc, B, ham in shapes:
        B = max(1, int(B * scale))
        eng = tq.VQEEngine(n)
        eng.set_hamiltonian(*ham)
        circs, ths = circuits(n, P, nc, B, rng)
        eng.batch_load(circs, ths)
        eng.batch_set_new_gate([len(c) - 1 for c in circs])
        rec = {"name": name, "n": n, "P": P, "B": B}
        for label, run in (("cobyla", lambda: eng.batch_run_env_step(1.0, 1e-4, budget)),
                           ("spsa", lambda: eng.batch_run_env_step_spsa(maxiter=K))):
            ms = timed(eng, run, reps)
            _, f, nfev = eng.batch_fetch(want_x=False)
            med = float(np.median(ms))
            rec[label] = {"ms": ms, "median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)),
                          "mean_nfev": float(nfev.mean()), "evaluations_per_s": float(nfev.sum() / med * 1e3),
                          "mean_energy": float(f.mean()), "wg_per_cu": int(eng.device_info()["wg_per_cu"])}
            r = rec[label]
            rows.append(f"| {name} | {B} | {label} | {med:.2f} ({r['min_ms']:.2f} … {r['max_ms']:.2f}) | {r['mean_nfev']:.1f} | "
                        f"{r['evaluations_per_s'] / 1e6:.2f} M | {r['mean_energy']:+.5f} |")
            print(rows[-1], flush=True)
        out["shapes"].append(rec)
        eng.close()
    # depolarising noise: where does each optimiser end, measured by the channel itself
    n, P, nc, B = 8, 24, 8, 64
    circs, ths = circuits(n, P, nc, B, rng)
    noisy = [with_noise_gates(c) for c in circs]
    eng = tq.VQEEngine(n)
    eng.set_hamiltonian(*h2o)
    eng.set_noise(0.01, 0.05, 7)
    exact = tq.VQEEngine(n)
    exact.set_hamiltonian(*h2o)
    exact.set_noise(0.01, 0.05, 7)
    exact.set_noise_mode(1)

    def channel_energy(x):
        exact.batch_load(noisy, np.split(x, B))
        exact.batch_run_energy()
        return exact.batch_fetch(want_x=False)[1]

    rec = {"n": n, "P": P, "B": B, "p1": 0.01, "p2": 0.05, "start": float(channel_energy(np.concatenate(ths)).mean())}
    eng.batch_load(noisy, ths)
    for label, run in (("cobyla", lambda: eng.batch_run_minimize(1.0, 1e-4, budget)),
                       ("spsa", lambda: eng.batch_run_minimize_spsa(maxiter=K))):
        run()
        x, f, nfev = eng.batch_fetch()
        e = channel_energy(x)
        rec[label] = {"mean_exact_energy": float(e.mean()), "std_exact_energy": float(e.std()), "mean_nfev": float(nfev.mean()),
                      "mean_reported_energy": float(f.mean())}
        print(f"noise 8q P={P} B={B} {label}: mean exact-channel energy {e.mean():+.5f} (start {rec['start']:+.5f}), "
              f"mean nfev {nfev.mean():.1f}", flush=True)
    out["noise"] = rec
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "spsa.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print("| shape | B | optimiser | ms per launch: median (min … max) | mean nfev | evaluations/s | mean E |")
    print("|---|---|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
