"""Mode 0 Pauli noise: the adjoint gradient and the device L-BFGS on frozen realisations (vqe_set_noise_grad, DESIGN.md
4.20) beside the noiseless adjoint kernels and the noisy device COBYLA, at n = 8 and 12 qubits and T = 1, 4, 16.

Workload per point: B = 256 circuits of 40 random gates (CNOT / RX / RY / RZ) with a depolarising channel behind every
gate (p1 = 0.01, p2 = 0.05), Heisenberg chain.  Wall clock around the library calls (run + fetch), three repeats after
one warm-up run each:
  noisy_gradient_s      one gradient run on T frozen realisations (batch_run_energy_grad, the NOISY instance)
  noiseless_T_s         T x one gradient run of the same circuits with p1 = p2 = 0 (the noiseless instance, whose code
                        the switch does not change: what the T sweeps cost without the noise slots, the patch and the
                        accumulation)
  env-steps             batch_load + batch_set_new_gate + one env-step + fetch: the noisy device COBYLA (one draw per
                        evaluation, maxfun 40) and the device L-BFGS on T frozen realisations (maxfun 40)
  end_energy            where each env-step ends: the mean over the batch of the mean energy of 256 fresh realisations
                        (a seed of their own) of the full circuits at the returned parameters
Every n runs in a child process of its own under a time limit; a child that fails or runs out of time ends the probe.
Writes profiles/noise_grad.json (--out).  Started by hand; not a test."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, REALS, BATCH, REPEATS, GATES, MAXFUN, FRESH = (8, 12), (1, 4, 16), 256, 3, 40, 40, 256
P1, P2 = 0.01, 0.05
STEP_LIMIT_S = 400


def worker(n):
    sys.path.insert(0, ROOT)
    import numpy as np
    import tensorrl_qas_amd as tq
    rng = np.random.default_rng(2044 + n)
    ham, _ = tq.hamiltonian.heisenberg(n)
    eng = tq.VQEEngine(n)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    circs, ths, new = [], [], []
    for _ in range(BATCH):
        c, th = tq.circuits.random_circuit(n, GATES, rng)
        k, a, b, p = [], [], [], []
        for kk, aa, bb, pp in zip(c.kind, c.q0, c.q1, c.pidx):
            k += [int(kk), 5 if kk == 0 else 4]; a += [int(aa), int(aa)]; b += [int(bb), int(bb) if kk == 0 else -1]; p += [int(pp), -1]
        th = np.asarray(th, np.float32).astype(np.float64)
        g = max(i for i, kk in enumerate(k) if kk < 4)
        if k[g] != 0:
            th[p[g]] = 0.0
        circs.append(tq.Circuit(k, a, b, p, th.size)), ths.append(th), new.append(g)
    sizes = [t.size for t in ths]

    def timed(fn):
        fn()
        out = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            r = fn()
            out.append(time.perf_counter() - t0)
        return out, r

    def gradient():
        eng.batch_run_energy_grad()
        return eng.batch_fetch(want_x=False), eng.batch_fetch_grad()

    def env_step(lbfgs):
        def run():
            eng.batch_load(circs, ths)
            eng.batch_set_new_gate(new)
            if lbfgs:
                eng.batch_run_env_step_lbfgs(maxfun=MAXFUN)
            else:
                eng.batch_run_env_step(1.0, 1e-4, MAXFUN)
            return eng.batch_fetch()
        return run

    def end_energy(x):
        """mean over the batch of the mean of FRESH single-draw energies of the full circuits at x"""
        eng.set_noise(P1, P2, 99)
        eng.batch_load(circs, list(np.split(x, np.cumsum(sizes)[:-1])))
        tot = 0.0
        for _ in range(FRESH):
            eng.batch_run_energy()
            tot += float(eng.batch_fetch(want_x=False)[1].mean())
        return tot / FRESH

    med = lambda v: sorted(v)[REPEATS // 2]
    # the noisy device COBYLA env-step does not depend on T
    eng.set_noise(P1, P2, 1)
    eng.set_noise_grad(0)
    tc, (xc, fc, nc) = timed(env_step(False))
    cobyla = {"s": tc, "reported_energy": float(fc.mean()), "mean_nfev": float(nc.mean()), "end_energy": end_energy(xc)}
    for T in REALS:
        eng.set_noise(0.0, 0.0, 1)
        eng.set_noise_grad(T)
        eng.batch_load(circs, ths)
        t1, _ = timed(gradient)
        clean_T = [t * T for t in t1]
        eng.set_noise(P1, P2, 1)
        eng.batch_load(circs, ths)
        tg, _ = timed(gradient)
        wg = eng.device_info()["wg_per_cu"]
        tl, (xl, fl, nl) = timed(env_step(True))
        print(json.dumps({
            "n": n, "T": T, "B": BATCH, "wg_per_cu": wg, "noisy_gradient_s": tg, "noiseless_gradient_s": t1, "noiseless_T_s": clean_T,
            "noisy_over_T_noiseless": med(tg) / med(clean_T),
            "env_step_cobyla": cobyla,
            "env_step_lbfgs": {"s": tl, "reported_energy": float(fl.mean()), "mean_nfev": float(nl.mean()), "end_energy": end_energy(xl)},
        }), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_grad.json"))
    ap.add_argument("--worker", metavar="N", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(int(args.worker))
    points = []
    for n in SIZES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(n)], capture_output=True, text=True,
                               timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"n={n}: no result within {STEP_LIMIT_S} s - probe ended")
        if r.returncode != 0:
            sys.exit(f"n={n}: exit status {r.returncode} - probe ended\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                p = json.loads(line)
                points.append(p)
                c, l = p["env_step_cobyla"], p["env_step_lbfgs"]
                print(f"n={p['n']:2d} T={p['T']:2d}: noisy gradient {sorted(p['noisy_gradient_s'])[1] * 1e3:.2f} ms = x{p['noisy_over_T_noiseless']:.2f} of "
                      f"T noiseless ones; env-step COBYLA {sorted(c['s'])[1] * 1e3:.1f} ms ends at {c['end_energy']:.6f}, "
                      f"L-BFGS {sorted(l['s'])[1] * 1e3:.1f} ms ends at {l['end_energy']:.6f}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/probe_noise_grad.py", "gates": GATES, "channels": GATES, "p1": P1, "p2": P2, "maxfun": MAXFUN,
                   "batch": BATCH, "fresh_realisations": FRESH, "repeats": REPEATS, "points": points}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
