"""Exact channel mode: the batched lock-step path (vqe_set_dm_batched) beside the serial host-driven path
AS BUILT FROM THE PARENT COMMIT, at n = 6, 8, 10 qubits and batches of 1, 8 and 64 circuits.

The serial figures are not read off the library under test: build the commit before this feature into a scratch
directory and pass its library,

    git archive <parent commit> | tar -x -C <scratch> && make -C <scratch>/tensorrl-qas_amd/csrc ../libvqe_hip.so
    python tools/probe_dm_batch.py --parent-lib <scratch>/tensorrl-qas_amd/libvqe_hip.so

Workload per point: B circuits of 20 random gates (CNOT / RX / RY / RZ) with a depolarising channel behind every gate
(p1 = 0.01, p2 = 0.05), Heisenberg chain.  Two figures, wall clock around the library calls (the serial path's cost is
host work between its launches, which device events do not see), three repeats after one warm-up run each:
  evaluations/s   B / time of batch_run_energy + fetch
  env-steps/s     B / time of batch_load + batch_set_new_gate + batch_run_env_step(1.0, 1e-4, 40) + fetch
Every (library, n) pair runs in a child process of its own under a time limit; a child that fails or runs out of time
ends the probe.  Writes profiles/dm_batch.json (--out).  Started by hand; not a test."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, BATCHES, REPEATS, GATES, MAXFUN = (6, 8, 10), (1, 8, 64), 3, 20, 40
STEP_LIMIT_S = 300


def worker(variant, n):
    sys.path.insert(0, ROOT)
    import numpy as np
    from tensorrl_qas_amd import _lib
    if variant == "serial":      # the parent's library has no such symbols: the binding must not ask for them
        _lib.SIGNATURES.pop("vqe_set_dm_batched", None)
        _lib.SIGNATURES.pop("vqe_dm_batch_info", None)
    import tensorrl_qas_amd as tq
    rng = np.random.default_rng(2031 + n)
    ham, _ = tq.hamiltonian.heisenberg(n)
    eng = tq.VQEEngine(n)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    eng.set_noise(0.01, 0.05, 1)
    eng.set_noise_mode(1)
    if variant == "batched":
        eng.set_dm_batched(-1)
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

        def energy():
            eng.batch_run_energy()
            return eng.batch_fetch(want_x=False)

        def env_step():
            eng.batch_load(circs, ths)
            eng.batch_set_new_gate(new)
            eng.batch_run_env_step(1.0, 1e-4, MAXFUN)
            return eng.batch_fetch()

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
        ts, (_, f, nfev) = timed(env_step)
        info = eng.dm_batch_info() if variant == "batched" else None
        print(json.dumps({"variant": variant, "n": n, "B": B, "evaluations_per_s": [B / t for t in te],
                          "env_steps_per_s": [B / t for t in ts], "mean_nfev": float(nfev.mean()), "mean_energy": float(f.mean()),
                          "batch_info": info}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libvqe_hip.so built from the parent commit (the serial path)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dm_batch.json"))
    ap.add_argument("--worker", nargs=2, metavar=("VARIANT", "N"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]))
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: the library built from the parent commit is needed (see the module docstring)")
    points = []
    for n in SIZES:
        for variant in ("serial", "batched"):
            env = dict(os.environ)
            if variant == "serial":
                env["VQE_HIP_LIB"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("VQE_HIP_LIB", None)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", variant, str(n)], env=env, capture_output=True,
                                   text=True, timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired:
                sys.exit(f"{variant} n={n}: no result within {STEP_LIMIT_S} s - probe ended")
            if r.returncode != 0:
                sys.exit(f"{variant} n={n}: exit status {r.returncode} - probe ended\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    points.append(json.loads(line))
                    print(line, flush=True)
    table = []
    for n in SIZES:
        for B in BATCHES:
            s = next(p for p in points if (p["variant"], p["n"], p["B"]) == ("serial", n, B))
            b = next(p for p in points if (p["variant"], p["n"], p["B"]) == ("batched", n, B))
            row = {"n": n, "B": B}
            for key in ("evaluations_per_s", "env_steps_per_s"):
                row[key] = {"serial_parent": s[key], "batched": b[key],
                            "ratio_of_medians": sorted(b[key])[REPEATS // 2] / sorted(s[key])[REPEATS // 2],
                            "batched_not_slower_beyond_spread": max(b[key]) >= min(s[key])}
            row["mean_nfev"] = {"serial_parent": s["mean_nfev"], "batched": b["mean_nfev"]}
            table.append(row)
            print(f"n={n:2d} B={B:2d}: evaluations/s x{row['evaluations_per_s']['ratio_of_medians']:.2f}, "
                  f"env-steps/s x{row['env_steps_per_s']['ratio_of_medians']:.2f}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/probe_dm_batch.py", "gates": GATES, "channels": GATES, "p1": 0.01, "p2": 0.05, "maxfun": MAXFUN,
                   "repeats": REPEATS, "points": points, "table": table}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
