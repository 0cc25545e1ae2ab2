"""Adjoint gradient (vqe_batch_run_energy_grad) against energies (vqe_batch_run_energy) and parameter shift (2P+1
energies per gradient) at the trainable-regime sizes: 8 qubits / H2O-8q with 129 parameters, 12 qubits / synthetic
LiH-12q with 202 parameters; B = 512 and 4096 circuits.  Kernel times by HIP events on the handle's stream (median of
five launches after two warm-up launches).  The parameter-shift column is (2P+1) x the energy launch of the same
batch: one gradient by shifts is exactly that many energy evaluations.  usage: probe_grad.py [B ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensorrl_qas_amd as tq  # noqa: E402


def circuits(n, P, n_cnot, B, rng):
    out, ths = [], []
    for _ in range(B):
        kind = np.array([0] * n_cnot + list(rng.integers(1, 4, P)), np.int32)
        rng.shuffle(kind)
        q0 = rng.integers(0, n, kind.size).astype(np.int32)
        q1 = np.where(kind == 0, (q0 + 1 + rng.integers(0, n - 1, kind.size)) % n, -1).astype(np.int32)
        pidx = np.where(kind > 0, np.cumsum(kind > 0) - 1, -1).astype(np.int32)
        out.append(tq.Circuit(kind, q0, q1, pidx, P))
        ths.append(rng.uniform(-np.pi, np.pi, P))
    return out, ths


def timed(eng, run, reps=5):
    for _ in range(2):
        run()
    eng.sync()
    ms = []
    for _ in range(reps):
        run()
        eng.sync()
        ms.append(eng.last_kernel_ms())
    return float(np.median(ms))


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [512, 4096]
    d = np.load(os.path.join(ROOT, "tests", "golden", "ham_H2O_8q.npz"))
    xs, zs = tq.hamiltonian.masks_from_strings([str(s) for s in d["paulis"]], 8)
    lih = tq.hamiltonian.synthetic_lih12()
    problems = [(8, 129, 21, (xs, zs, np.asarray(d["weights"], float))), (12, 202, 37, (lih.xmask, lih.zmask, lih.coeff))]
    rng = np.random.default_rng(2024)
    for n, P, nc, ham in problems:
        eng = tq.VQEEngine(n)
        eng.set_hamiltonian(*ham)
        for B in sizes:
            circs, ths = circuits(n, P, nc, B, rng)
            eng.batch_load(circs, ths)
            t_e = timed(eng, eng.batch_run_energy)
            t_g = timed(eng, eng.batch_run_energy_grad)
            wg = eng.device_info()["wg_per_cu"]
            t_ps = (2 * P + 1) * t_e
            print(f"n={n:2d} P={P} B={B:5d}: energy {t_e:8.3f} ms  adjoint E+grad {t_g:8.3f} ms ({t_g / t_e:5.2f} x energy, "
                  f"wg/CU {wg})  parameter shift {t_ps:9.1f} ms ({t_ps / t_g:6.1f} x adjoint)  "
                  f"{B / t_g * 1e3:10.0f} gradients/s", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
