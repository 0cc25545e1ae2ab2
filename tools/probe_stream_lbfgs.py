"""Device L-BFGS of the streaming path (vqe_set_stream_lbfgs, vqe_batch_run_minimize_lbfgs) beside the streaming device
COBYLA (vqe_batch_run_minimize) on the shapes of probe_stream_grad.py: Heisenberg chains at n = 16, 18, 20, P = 40
rotations and 20 CNOTs per circuit, batches of 16, 8 and 4 streams.  Three runs per size from the same start points:
COBYLA at maxfun = 200, L-BFGS at maxfun = 200 and at maxfun = 50 (maxiter = maxfun, the other options default).
Reported per run: last_kernel_ms (the whole optimiser run by HIP events on the handle's stream, median of five runs
after two warm-up runs), mean nfev, mean final energy, and per L-BFGS run the share of streams on which it ends lower
than COBYLA / COBYLA ends lower than it.
--cobyla-only: the COBYLA column alone; runs on a library without vqe_set_stream_lbfgs (VQE_HIP_LIB=<older build>).
usage: probe_stream_lbfgs.py [--cobyla-only] [n ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensorrl_qas_amd as tq  # noqa: E402
from tensorrl_qas_amd import _lib  # noqa: E402
from probe_grad import circuits, timed  # noqa: E402

BATCH = {16: 16, 18: 8, 20: 4}


def main():
    args = sys.argv[1:]
    cobyla_only = "--cobyla-only" in args
    if cobyla_only:      # an older library has no such symbol: the binding must not ask for it
        _lib.SIGNATURES.pop("vqe_set_stream_lbfgs", None)
    sizes = [int(a) for a in args if not a.startswith("--")] or [16, 18, 20]
    P, n_cnot = 40, 20
    rng = np.random.default_rng(2026)
    for n in sizes:
        B = BATCH.get(n, 4)
        ham, _ = tq.hamiltonian.heisenberg(n)
        eng = tq.VQEEngine(n)
        eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
        circs, ths = circuits(n, P, n_cnot, B, rng)
        eng.batch_load(circs, ths)

        def column(name, run):
            ms = timed(eng, run)
            _, f, nfev = eng.batch_fetch()
            print(f"n={n:2d} P={P} B={B:3d} {name:<18s}: {ms:9.2f} ms  mean nfev {nfev.mean():6.1f}  mean E {f.mean():+.6f}", flush=True)
            return f

        f_c = column("COBYLA maxfun=200", lambda: eng.batch_run_minimize(maxfun=200))
        if not cobyla_only:
            eng.set_stream_lbfgs()
            for mf in (200, 50):
                f_l = column(f"L-BFGS maxfun={mf}", lambda mf=mf: eng.batch_run_minimize_lbfgs(maxfun=mf, maxiter=mf))
                nit, st = eng.batch_fetch_lbfgs_info()
                print(f"{'':14s} L-BFGS lower on {np.mean(f_l < f_c):4.0%} of the streams, COBYLA lower on {np.mean(f_c < f_l):4.0%}; "
                      f"mean nit {nit.mean():5.1f}, status counts {np.bincount(st, minlength=5).tolist()}", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
