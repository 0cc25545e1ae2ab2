"""GPU, several ranks on the ONE card of the test box (gloo): collected last (conftest.py), so that a failure of
the multi-process harness can never hide the single-process parity suites under ``pytest -x``.  The ranks are
fresh interpreters started by tests/rank_workers.py; this process is never forked."""
import numpy as np
import pytest

import vqe_oracle as vo
from helpers import random_gates, random_hamiltonian, random_state

pytestmark = pytest.mark.gpu


def test_term_sharded_engine_two_ranks_on_one_gpu(tmp_path):
    """world_size 2 (gloo, both ranks on cuda:0): all-reduced energies equal the unsharded energy,
    the lock-step sharded COBYLA returns the same x / f / nfev on both ranks, and f is the
    (unscaled) energy at x."""
    from rank_workers import run_ranks
    r0, r1 = run_ranks("sharded_gpu", 2, tmp_path)
    assert set(r0) == {"12_0", "14_1", "14_0"}
    for key in r0:
        n = int(key.split("_")[0])
        rng = np.random.default_rng(n)
        psi0 = random_state(n, rng)
        ham = random_hamiltonian(n, 30, rng)
        kind, q0, q1, pidx, th = random_gates(n, 10, rng)
        assert r0[key] == r1[key]
        assert abs(r0[key]["e"] - vo.energy_pauli(vo.run_circuit(psi0, kind, q0, q1, pidx, th), *ham)) < 1e-10
        x = np.array(r0[key]["x"])
        assert abs(r0[key]["f"] - vo.energy_pauli(vo.run_circuit(psi0, kind, q0, q1, pidx, x), *ham)) < 1e-10
        assert 1 <= r0[key]["nfev"] <= 40


def test_amplitude_sharded_states_two_processes_cuda_shards(tmp_path):
    """world_size 2 (gloo, both ranks on cuda:0), one CUDA shard of a 15-qubit register per process on a 14-qubit
    handle: the cross-process branch of AmplitudeShardedState._exchange (send / recv through the host, copy back to
    the device) with every exchange 30 ms late on its stream.  Both ranks report the same total, it is the oracle's
    energy, and each rank sent half a shard per exchange."""
    from rank_workers import AMP_GPU_CASE, run_ranks
    from stream_order_helpers import MIN_DELAY_MS, heisenberg_case
    n, G, seed = AMP_GPU_CASE
    case = heisenberg_case(n, 2, G, seed)
    r0, r1 = run_ranks("amp_sharded_gpu", 2, tmp_path, timeout=120)
    print("ranks:", r0, r1, "oracle:", case["e"])
    for r in (r0, r1):
        assert r["shard"] == 1 << 14 and r["swaps"] == case["swaps"] >= 1
        assert r["delays"] == 2 * r["swaps"] and r["min_delay_ms"] >= MIN_DELAY_MS      # before the send, before the copy back
        assert r["bytes"] == r["swaps"] * (1 << 14) * 8
    assert r0["total"] == r1["total"]
    assert abs(r0["total"] - case["e"]) < 1e-10
    assert abs(r0["part"] + r1["part"] - r0["total"]) < 1e-12
