"""Device L-BFGS (vqe_batch_run_minimize_lbfgs) against device COBYLA (vqe_batch_run_minimize) on three shapes:
trainable 8 qubits / H2O-8q / 129 variables / B = 4096, trainable 12 qubits / synthetic LiH-12q / 202 variables / B = 512,
fixed 12 qubits / 32 variables / B = 4096.  Per shape: COBYLA at maxfun = 1000, L-BFGS at maxfun = 1000 and at
maxfun = 100 (maxiter = maxfun, so that the evaluation budget is the binding one; the other options are the defaults).
Kernel times by HIP events on the handle's stream, median of five launches after two warm-up launches; every launch
starts from the same x0.  Reported: launch time, mean nfev, mean final energy, and the share of circuits on which each
optimiser ends lower than COBYLA / the L-BFGS.
usage: probe_lbfgs.py [--cobyla-only] [--scale S]   (--scale: multiply every B by S, for quick runs;
--cobyla-only: the COBYLA column alone, which also runs on a library without the L-BFGS entry points)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensorrl_qas_amd as tq  # noqa: E402
from probe_grad import circuits, timed  # noqa: E402


def main():
    args = sys.argv[1:]
    cobyla_only = "--cobyla-only" in args
    scale = float(args[args.index("--scale") + 1]) if "--scale" in args else 1.0
    d = np.load(os.path.join(ROOT, "tests", "golden", "ham_H2O_8q.npz"))
    xs, zs = tq.hamiltonian.masks_from_strings([str(s) for s in d["paulis"]], 8)
    h2o = (xs, zs, np.asarray(d["weights"], float))
    lih = tq.hamiltonian.synthetic_lih12()
    lih = (lih.xmask, lih.zmask, lih.coeff)
    shapes = [("trainable  8q P=129", 8, 129, 21, 4096, h2o), ("trainable 12q P=202", 12, 202, 37, 512, lih),
              ("fixed     12q P= 32", 12, 32, 12, 4096, lih)]
    rng = np.random.default_rng(2025)
    for name, n, P, nc, B, ham in shapes:
        B = max(1, int(B * scale))
        eng = tq.VQEEngine(n)
        eng.set_hamiltonian(*ham)
        circs, ths = circuits(n, P, nc, B, rng)
        eng.batch_load(circs, ths)
        runs = [("COBYLA  maxfun=1000", lambda: eng.batch_run_minimize(1.0, 1e-4, 1000))]
        if not cobyla_only:
            runs += [("L-BFGS  maxfun=1000", lambda: eng.batch_run_minimize_lbfgs(maxfun=1000, maxiter=1000)),
                     ("L-BFGS  maxfun= 100", lambda: eng.batch_run_minimize_lbfgs(maxfun=100, maxiter=100))]
        res = []
        for label, run in runs:
            ms = timed(eng, run)
            _, f, nfev = eng.batch_fetch(want_x=False)
            st = eng.batch_fetch_lbfgs_info()[1] if label.startswith("L-BFGS") else None
            res.append((label, ms, f.copy(), nfev.copy(), st))
        f_cob = res[0][2]
        for label, ms, f, nfev, st in res:
            line = (f"{name} B={B:5d}  {label}: {ms:10.2f} ms  mean nfev {nfev.mean():7.1f}  mean E {f.mean():+.6f}  "
                    f"{B * nfev.mean() / ms * 1e3:12.0f} evaluations/s")
            if f is not f_cob:
                line += (f"  lower than COBYLA on {100.0 * np.mean(f < f_cob - 1e-9):5.1f} %, higher on "
                         f"{100.0 * np.mean(f > f_cob + 1e-9):5.1f} %")
                line += "  status counts " + str(np.bincount(st, minlength=5).tolist())
            print(line, flush=True)
        eng.close()


if __name__ == "__main__":
    main()
