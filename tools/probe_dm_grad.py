"""Exact channel mode: the adjoint gradient and the device L-BFGS of the batched path (vqe_set_dm_grad)
beside that path's own energies and device COBYLA, at n = 6, 8, 10 qubits and batches of 1, 8 and 64 circuits.

Workload per point: the circuits of tools/probe_dm_batch.py - B circuits of 20 random gates (CNOT / RX / RY / RZ) with a
depolarising channel behind every gate (p1 = 0.01, p2 = 0.05), Heisenberg chain.  Wall clock around the library calls,
three repeats after one warm-up run each:
  energy_s          one batched energy evaluation (batch_run_energy + fetch)
  gradient_s        one batched gradient evaluation (batch_run_energy_grad + fetch of E and the gradient)
  shift_s           the same gradient by parameter shift on the batched energies: 2 x rotations energy evaluations of the
                    batch (every rotation of these circuits has an angle of its own; the circuits of a batch are shifted
                    side by side, the longest one sets the count)
  bytes_per_s       4^n x 16 bytes x passes / time: an energy evaluation makes 2 passes per level (read, write), a gradient
                    evaluation 6 (forward 2, M 2, Lambda 2) - levels from dm_batch_info
  env-steps         batch_load + batch_set_new_gate + one env-step + fetch with the device COBYLA (maxfun 40) and with the
                    device L-BFGS (maxfun 40): time, mean final energy, lock-step evaluations (dm_batch_info)
Every n runs in a child process of its own under a time limit; a child that fails or runs out of time ends the probe.
Writes profiles/dm_grad.json (--out).  Started by hand; not a test."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, BATCHES, REPEATS, GATES, MAXFUN = (6, 8, 10), (1, 8, 64), 3, 20, 40
STEP_LIMIT_S = 300


def worker(n):
    sys.path.insert(0, ROOT)
    import numpy as np
    import tensorrl_qas_amd as tq
    rng = np.random.default_rng(2031 + n)
    ham, _ = tq.hamiltonian.heisenberg(n)
    eng = tq.VQEEngine(n)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    eng.set_noise(0.01, 0.05, 1)
    eng.set_noise_mode(1)
    eng.set_dm_batched(-1)
    eng.set_dm_grad()
    for B in BATCHES:
        circs, ths, new = [], [], []
        for _ in range(B):
            c, th = tq.circuits.random_circuit(n, GATES, rng)
            k, a, b, p = [], [], [], []
            for kk, aa, bb, pp in zip(c.kind, c.q0, c.q1, c.pidx):
                k += [int(kk), 5 if kk == 0 else 4]; a += [int(aa), int(aa)]; b += [int(bb), int(bb) if kk == 0 else -1]; p += [int(pp), -1]
            th = np.asarray(th, np.float32).astype(np.float64)
            g = max(i for i, kk in enumerate(k) if kk < 4)
            if k[g] != 0:
                th[p[g]] = 0.0
            circs.append(tq.Circuit(k, a, b, p, th.size)), ths.append(th), new.append(g)
        rotations = max(t.size for t in ths)

        def energy():
            eng.batch_run_energy()
            return eng.batch_fetch(want_x=False)

        def gradient():
            eng.batch_run_energy_grad()
            return eng.batch_fetch(want_x=False), eng.batch_fetch_grad()

        def shift():
            for j in range(rotations):
                for sign in (1.0, -1.0):
                    moved = [t.copy() for t in ths]
                    for t in moved:
                        if j < t.size:
                            t[j] += sign * np.pi / 2
                    eng.batch_load(circs, moved)
                    eng.batch_run_energy()
                    eng.batch_fetch(want_x=False)
            eng.batch_load(circs, ths)

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

        def timed(fn):
            fn()
            out = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                r = fn()
                out.append(time.perf_counter() - t0)
            return out, r

        eng.batch_load(circs, ths)
        te, _ = timed(energy)
        info_e = eng.dm_batch_info()
        tg, _ = timed(gradient)
        info_g = eng.dm_batch_info()
        tsh, _ = timed(shift)
        tc, (_, fc, nc) = timed(env_step(False))
        info_c = eng.dm_batch_info()
        tl, (_, fl, nl) = timed(env_step(True))
        info_l = eng.dm_batch_info()
        dm_bytes = 16.0 * 4 ** n
        med = lambda v: sorted(v)[REPEATS // 2]
        print(json.dumps({
            "n": n, "B": B, "rotations": rotations, "levels": info_g["levels"], "resident_energy": info_e["resident"],
            "resident_gradient": info_g["resident"], "energy_s": te, "gradient_s": tg, "shift_s": tsh,
            "gradient_over_energy": med(tg) / med(te), "shift_over_gradient": med(tsh) / med(tg),
            "energy_bytes_per_s": B * dm_bytes * 2 * info_e["levels"] / med(te),
            "gradient_bytes_per_s": B * dm_bytes * 6 * info_g["levels"] / med(tg),
            "env_step_cobyla": {"s": tc, "mean_energy": float(fc.mean()), "mean_nfev": float(nc.mean()), "evaluations": info_c["evaluations"]},
            "env_step_lbfgs": {"s": tl, "mean_energy": float(fl.mean()), "mean_nfev": float(nl.mean()), "evaluations": info_l["evaluations"]},
        }), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dm_grad.json"))
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
                print(f"n={p['n']:2d} B={p['B']:2d}: gradient / energy x{p['gradient_over_energy']:.2f}, shift / gradient "
                      f"x{p['shift_over_gradient']:.1f} ({p['rotations']} rotations), env-step COBYLA {sorted(p['env_step_cobyla']['s'])[1] * 1e3:.1f} ms "
                      f"E={p['env_step_cobyla']['mean_energy']:.6f}, L-BFGS {sorted(p['env_step_lbfgs']['s'])[1] * 1e3:.1f} ms "
                      f"E={p['env_step_lbfgs']['mean_energy']:.6f}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/probe_dm_grad.py", "gates": GATES, "channels": GATES, "p1": 0.01, "p2": 0.05, "maxfun": MAXFUN,
                   "repeats": REPEATS, "points": points}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
