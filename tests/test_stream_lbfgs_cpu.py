"""CPU: the cases tests/test_stream_lbfgs_gpu.py compares with the restatement of the device L-BFGS have no marginal
decision and do not hang on the last digits of a gradient, they cover a backtracking trial and an eviction, the batch
case has streams that stop at different evaluations on both sides of the host's polling interval, and the library
exports the switch of the streaming path."""
import numpy as np
import pytest

import lbfgs_helpers as lh
import stream_lbfgs_helpers as sh


@pytest.mark.parametrize("n,seed", sh.CASES)
def test_compared_cases_have_no_marginal_decision(n, seed):
    case = sh.single_case(n, seed)
    r = sh.restated_single(n, seed)
    assert r.marginal == [], r.marginal
    assert r.nit >= 1 and r.nfev == len(r.trials)
    assert all(abs(t.slack) >= 1e-8 * case["scale"] for t in r.trials[1:])
    sens = lh.gradient_sensitivity(case, r, **sh.TRAJ_OPTS)
    assert sens <= lh.X_SENSITIVITY_MAX, sens


def test_compared_cases_cover_backtracking_and_eviction():
    runs = [sh.restated_single(n, seed) for n, seed in sh.CASES]
    assert any(r.nfev > r.nit + 1 for r in runs), [(r.nfev, r.nit) for r in runs]
    assert any(r.evictions > 0 for r in runs), [r.evictions for r in runs]


def test_a_prefix_is_the_full_run_cut_at_maxfun():
    """What the GPU test relies on: maxfun = k evaluates the first k points of the full run, k = 1 is x0 with status 3."""
    n, seed = sh.CASES[2]
    full = sh.restated_single(n, seed)
    for k in range(1, full.nfev + 1):
        r = sh.restated_single(n, seed, maxfun=k)
        assert r.nfev == k and r.marginal == []
        assert all(np.array_equal(a.x, b.x) for a, b in zip(r.trials, full.trials))
        assert r.status == (lh.MAXFUN if k < full.nfev else full.status)
    first = sh.restated_single(n, seed, maxfun=1)
    assert np.array_equal(first.x, sh.single_case(n, seed)["theta"]) and first.nit == 0


def test_batch_case_streams_stop_at_different_evaluations():
    nfev = [sh.batch_restated(b).nfev for b in range(4)]
    assert len(set(nfev)) > 1, nfev
    assert min(nfev) <= max(nfev) - 3, nfev                  # one stream is finished while the others go on
    assert max(nfev) > sh.STREAM_POLL, nfev                  # the longest one runs past a look at the running count
    ng = sh.batch_new_gates()
    kinds = [c["gates"][0] for c in sh.batch_case()["circuits"]]
    assert kinds[0][ng[0]] != 0 and kinds[1][ng[1]] == 0 and ng[2] == -1 and kinds[3][ng[3]] != 0
    hole = int(sh.batch_case()["circuits"][3]["gates"][3][ng[3]])
    assert 0 < hole < sh.batch_case()["circuits"][3]["theta"].size - 1      # variables on both sides of the hole


def test_library_exports_the_switch():
    """Needs no GPU: the library loads without one."""
    from tensorrl_qas_amd import _lib
    assert "vqe_set_stream_lbfgs" in _lib.SIGNATURES
    assert _lib.SIGNATURES["vqe_set_stream_lbfgs"] == _lib.SIGNATURES["vqe_set_stream_grad"]
    lib = _lib.load()
    assert lib.vqe_set_stream_lbfgs(None, 1) == -22           # VQE_EINVAL for a NULL handle
