"""What a two-qubit Pauli rotation costs the device: kernel time of vqe_batch_run_energy (HIP events on the handle's
stream, median of five launches after two warm-up launches) for batches of identical shape in three variants -
(a) G one-qubit rotations with CNOTs in between, (b) the same circuits with every RX replaced by RXX and every RY by RYY
on (qubit, a random partner), (c) variant (b) spelled as CNOT . R . CNOT (RYY with its four fixed RZ(+-pi/2)).  12 qubits
(register path, B circuits) and 20 qubits (streaming path, (a) against (b)).  usage: probe_su4.py [--only-a] [B12 [B20]]
(--only-a: variant (a) alone, for a library built before the two-qubit rotations existed)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tensorrl_qas_amd as tq  # noqa: E402


def variants(n, G, n_cnot, B, rng):
    """-> three lists of (Circuit, theta): (a), (b), (c)."""
    out = ([], [], [])
    for _ in range(B):
        kind = np.array([0] * n_cnot + list(rng.integers(1, 4, G)), np.int32)
        rng.shuffle(kind)
        q0 = rng.integers(0, n, kind.size).astype(np.int32)
        q1 = ((q0 + 1 + rng.integers(0, n - 1, kind.size)) % n).astype(np.int32)      # CNOT target / partner of (b)
        th = rng.uniform(-np.pi, np.pi, G)
        pidx = np.where(kind > 0, np.cumsum(kind > 0) - 1, -1).astype(np.int32)
        out[0].append((tq.Circuit(kind, q0, np.where(kind == 0, q1, -1), pidx, G), th))
        kb = np.where(kind == 1, 6, np.where(kind == 2, 7, kind)).astype(np.int32)
        out[1].append((tq.Circuit(kb, q0, np.where(kind == 3, -1, q1), pidx, G), th))
        k, a, b, p = [], [], [], []
        for kd, x, y, pi in zip(kind, q0, q1, pidx):
            if kd == 1:
                k += [0, 1, 0]; a += [x, x, x]; b += [y, -1, y]; p += [-1, pi, -1]
            elif kd == 2:
                k += [3, 3, 0, 1, 0, 3, 3]; a += [x, y, x, x, x, x, y]; b += [-1, -1, y, -1, y, -1, -1]
                p += [G, G, -1, pi, -1, G + 1, G + 1]
            else:
                k.append(kd); a.append(x); b.append(y if kd == 0 else -1); p.append(pi)
        out[2].append((tq.Circuit(k, a, b, p, G + 2), np.concatenate([th, [np.pi / 2, -np.pi / 2]])))
    return out


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
    args = [a for a in sys.argv[1:] if a != "--only-a"]
    only_a = "--only-a" in sys.argv[1:]
    b12 = int(args[0]) if len(args) > 0 else 4096
    b20 = int(args[1]) if len(args) > 1 else 16
    rng = np.random.default_rng(2025)
    lih = tq.hamiltonian.synthetic_lih12()
    h20, _ = tq.hamiltonian.heisenberg(20)
    for n, G, nc, B, ham, names in ((12, 48, 16, b12, lih, "abc"), (20, 24, 8, b20, h20, "ab")):
        eng = tq.VQEEngine(n)
        eng.set_hamiltonian(ham.xmask, ham.zmask, ham.coeff)
        vs = variants(n, G, nc, B, rng)
        t, e = {}, {}
        for name, v in zip("a" if only_a else names, vs):
            eng.batch_load([c for c, _ in v], [th for _, th in v])
            t[name] = timed(eng, eng.batch_run_energy)
            e[name] = eng.batch_fetch(want_x=False)[1]
        line = f"n={n} G={G} rotations + {nc} CNOT, B={B}: (a) one-qubit {t['a']:8.3f} ms"
        if "b" in t:
            line += f"  (b) RXX/RYY {t['b']:8.3f} ms ({t['b'] / t['a']:5.3f} x a)"
        if "c" in t:
            line += f"  (c) CNOT.R.CNOT {t['c']:8.3f} ms ({t['c'] / t['a']:5.3f} x a, {t['c'] / t['b']:5.3f} x b)"
            line += f"  max |E_b - E_c| {np.abs(e['b'] - e['c']).max():.1e}"
        print(line, flush=True)
        eng.close()


if __name__ == "__main__":
    main()
