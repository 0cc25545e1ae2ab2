"""The cases of the streaming-path device L-BFGS tests (tests/test_stream_lbfgs_gpu.py; k_sl_step of
tensorrl-qas_amd/csrc/vqe_stream_lbfgs.h behind vqe_set_stream_lbfgs, n >= 14), on the restatement and the oracle
objective of tests/lbfgs_helpers.py.  tests/test_stream_lbfgs_cpu.py checks on the CPU that every case compared with
the restatement has no marginal decision and passes the sensitivity bound.

There is no evaluation trace at n >= 14, so the GPU test compares PREFIXES: for k = 1 .. nfev the run with maxfun = k
against the restatement with the same maxfun.  Such a run evaluates the first k points of the full run, so the
objective is memoised per case and all prefixes together cost the evaluations of the full run."""
import numpy as np

import lbfgs_helpers as lh
from helpers import random_gates, random_hamiltonian, random_state

# (n, seed): 24 gates (p_cnot = 0.3), a random state, 12 complex Pauli terms, drawn in this order.  Seeds from
# 600 + n + 100 j; 714, 1014 (n = 14) and 715, 1015 (n = 15) fail the sensitivity bound and are left out.
CASES = [(14, 614), (14, 914), (14, 1114), (15, 815)]
TRAJ_OPTS = dict(lh.TRAJ_OPTS)                  # history 3, maxiter 6, maxfun 200
BATCH_OPTS = dict(history=2, maxiter=5)         # the batch case: compared with the library's own single runs
STREAM_POLL = 8                                 # kStreamPoll of csrc/vqe_api.hip: evaluations between two looks at the running count

_CASE, _FUN, _RESTATED = {}, {}, {}


def single_case(n, seed):
    """-> dict(n, psi0, gates = (kind, q0, q1, pidx), theta, ham, scale)"""
    if (n, seed) not in _CASE:
        rng = np.random.default_rng(seed)
        kind, q0, q1, pidx, th = random_gates(n, 24, rng, p_cnot=0.3)
        psi0 = random_state(n, rng)
        ham = random_hamiltonian(n, 12, rng, real=False)
        _CASE[(n, seed)] = dict(n=n, psi0=psi0, gates=(kind, q0, q1, pidx), theta=th, ham=ham, scale=lh.ham_scale(ham))
    return _CASE[(n, seed)]


def memo_fun(key, case):
    """lbfgs_helpers.oracle_fun of a case, every point evaluated once per process"""
    if key not in _FUN:
        fun = lh.oracle_fun(case["psi0"], *case["gates"], case["theta"].size, case["ham"])
        seen = {}

        def memo(x):
            k = np.asarray(x, np.float64).tobytes()
            if k not in seen:
                seen[k] = fun(x)
            f, g = seen[k]
            return f, g.copy()

        _FUN[key] = memo
    return _FUN[key]


def restated(key, case, **opts):
    """The restatement's run on a case with the given options, computed once per process"""
    full = (key, tuple(sorted(opts.items())))
    if full not in _RESTATED:
        _RESTATED[full] = lh.lbfgs(memo_fun(key, case), case["theta"], scale=case["scale"], **opts)
    return _RESTATED[full]


def restated_single(n, seed, maxfun=None):
    """The restated run of single_case(n, seed) under TRAJ_OPTS (maxfun: the prefix of that many evaluations)"""
    opts = dict(TRAJ_OPTS)
    if maxfun is not None:
        opts["maxfun"] = int(maxfun)
    return restated(("single", n, seed), single_case(n, seed), **opts)


def batch_case():
    """Four 14-qubit circuits of 10, 14, 18, 22 gates on one state and one Hamiltonian (seed 2014: the state, the
    Hamiltonian, then the circuits).  -> dict(n, psi0, ham, scale, circuits = [dict(gates, theta)])"""
    if "batch" not in _CASE:
        n = 14
        rng = np.random.default_rng(2014)
        psi0 = random_state(n, rng)
        ham = random_hamiltonian(n, 12, rng, real=False)
        circuits = []
        for b in range(4):
            kind, q0, q1, pidx, th = random_gates(n, 10 + 4 * b, rng, p_cnot=0.3)
            circuits.append(dict(gates=(kind, q0, q1, pidx), theta=th))
        _CASE["batch"] = dict(n=n, psi0=psi0, ham=ham, scale=lh.ham_scale(ham), circuits=circuits)
    return _CASE["batch"]


def batch_restated(b):
    """The restated run of circuit b of batch_case() under BATCH_OPTS"""
    case = batch_case()
    c = case["circuits"][b]
    sub = dict(psi0=case["psi0"], gates=c["gates"], theta=c["theta"], ham=case["ham"], scale=case["scale"])
    return restated(("batch", b), sub, **BATCH_OPTS)


def batch_new_gates():
    """The new gate of each circuit of batch_case() in the env-step test: the last rotation, the first CNOT, none, the
    rotation nearest the middle"""
    cs = batch_case()["circuits"]
    rot = [np.nonzero(c["gates"][0] != 0)[0] for c in cs]
    cnot1 = np.nonzero(cs[1]["gates"][0] == 0)[0]
    return [int(rot[0][-1]), int(cnot1[0]), -1, int(rot[3][rot[3].size // 2])]
