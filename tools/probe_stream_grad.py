"""Adjoint gradient of the streaming path (vqe_set_stream_grad, vqe_batch_run_energy_grad) against the energy launch
(vqe_batch_run_energy) and parameter shift (2P+1 energies per gradient) on Heisenberg chains at n = 16, 18, 20 with
P = 40 rotations and 20 CNOTs per circuit (an episode of BASELINE config 4 ends at 40 actions); batches of 16, 8 and
4 streams, so the states and their lambda copies stay at 32 MiB per stream at most.  Kernel times by HIP events on the
handle's stream (median of five launches after two warm-up launches).  The parameter-shift column is (2P+1) x the
energy launch of the same batch.  usage: probe_stream_grad.py [n ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensorrl_qas_amd as tq  # noqa: E402
from probe_grad import circuits, timed  # noqa: E402

BATCH = {16: 16, 18: 8, 20: 4}


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [16, 18, 20]
    P, n_cnot = 40, 20
    rng = np.random.default_rng(2026)
    for n in sizes:
        B = BATCH.get(n, 4)
        ham, _ = tq.hamiltonian.heisenberg(n)
        eng = tq.VQEEngine(n)
        eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
        eng.set_stream_grad()
        circs, ths = circuits(n, P, n_cnot, B, rng)
        eng.batch_load(circs, ths)
        t_e = timed(eng, eng.batch_run_energy)
        t_g = timed(eng, eng.batch_run_energy_grad)
        t_ps = (2 * P + 1) * t_e
        print(f"n={n:2d} P={P} B={B:3d}: energy {t_e:8.3f} ms  adjoint E+grad {t_g:8.3f} ms ({t_g / t_e:5.2f} x energy)  "
              f"parameter shift {t_ps:9.1f} ms ({t_ps / t_g:6.1f} x adjoint)", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
