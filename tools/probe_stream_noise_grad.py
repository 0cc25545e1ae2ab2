"""Gradients of frozen Pauli-noise realisations on the streaming path (vqe_set_stream_noise_grad): the
(circuit, realisation) grid beside the noiseless streaming gradient and beside its own serial form, at n = 14, 16 and 20
qubits, B = 1 and 8 circuits, T = 4 and 16 realisations.

Workload per point: B circuits of 40 random gates (CNOT / RX / RY / RZ) with a depolarising channel behind every gate
(p1 = 0.01, p2 = 0.05), Heisenberg chain.  Wall clock around the library calls (run + fetch), the median of three
repeats after one warm-up run each:
  noisy_s        one gradient run on T frozen realisations, max_resident = -1 (all B T pairs through one set of launches
                 where they fit)
  serial_s       the same with max_resident = 1: one pair per chunk, B T chunks
  noiseless_s    one gradient run of the same handle and circuits with p1 = p2 = 0 (the noiseless instances)
  ratio          noisy_s / (T x noiseless_s);  ratio_serial the same for serial_s
Every n runs in a child process of its own under a time limit; a child that fails or runs out of time ends the probe.
Writes profiles/stream_noise_grad.json (--out).  Started by hand; not a test."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, BATCHES, REALS, REPEATS, GATES = (14, 16, 20), (1, 8), (4, 16), 3, 40
P1, P2 = 0.01, 0.05
STEP_LIMIT_S = 300


def worker(n):
    sys.path.insert(0, ROOT)
    import numpy as np
    import tensorrl_qas_amd as tq
    rng = np.random.default_rng(2144 + n)
    ham, _ = tq.hamiltonian.heisenberg(n)
    eng = tq.VQEEngine(n)
    eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
    eng.set_stream_grad(True)
    circs, ths = [], []
    for _ in range(max(BATCHES)):
        c, th = tq.circuits.random_circuit(n, GATES, rng)
        k, a, b, p = [], [], [], []
        for kk, aa, bb, pp in zip(c.kind, c.q0, c.q1, c.pidx):
            k += [int(kk), 5 if kk == 0 else 4]; a += [int(aa), int(aa)]; b += [int(bb), int(bb) if kk == 0 else -1]; p += [int(pp), -1]
        circs.append(tq.Circuit(k, a, b, p, np.asarray(th).size)), ths.append(np.asarray(th, np.float64))

    def gradient():
        eng.batch_run_energy_grad()
        return eng.batch_fetch(want_x=False), eng.batch_fetch_grad()

    def timed():
        gradient()
        out = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            gradient()
            out.append(time.perf_counter() - t0)
        return out

    med = lambda v: sorted(v)[REPEATS // 2]
    for B in BATCHES:
        for T in REALS:
            eng.set_noise(0.0, 0.0, 1)
            eng.set_noise_grad(T, hold=True)
            eng.batch_load(circs[:B], ths[:B])
            clean = timed()
            eng.set_noise(P1, P2, 1)
            eng.set_stream_noise_grad(-1)
            grid = timed()
            info = eng.stream_noise_grad_info()
            eng.set_stream_noise_grad(1)
            serial = timed()
            print(json.dumps({"n": n, "B": B, "T": T, "resident": info["resident"], "chunks": info["chunks"],
                              "noisy_s": grid, "serial_s": serial, "noiseless_s": clean,
                              "ratio": med(grid) / (T * med(clean)), "ratio_serial": med(serial) / (T * med(clean))}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_noise_grad.json"))
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
                print(f"n={p['n']:2d} B={p['B']} T={p['T']:2d}: noisy {sorted(p['noisy_s'])[1] * 1e3:.2f} ms ({p['resident']} resident, "
                      f"{p['chunks']} chunks) = x{p['ratio']:.2f} of T noiseless ones ({sorted(p['noiseless_s'])[1] * 1e3:.2f} ms each); "
                      f"serial {sorted(p['serial_s'])[1] * 1e3:.2f} ms = x{p['ratio_serial']:.2f}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/probe_stream_noise_grad.py", "gates": GATES, "channels": GATES, "p1": P1, "p2": P2,
                   "repeats": REPEATS, "points": points}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
