"""Scenarios of the handle-reuse tests (tests/test_handle_reuse_cpu.py, tests/test_handle_reuse_gpu.py): ONE VQEEngine is
driven through a list of steps - some setters, then a run and its fetches - the way VecCircuitEnv keeps one vqe_t alive
for a whole training run.  After every step the GPU test compares the results with a FRESH handle that was given only
the step's final configuration (bit for bit) and with the oracle (the project's bounds).

This module builds the scenarios: inputs, the step list, what the reused handle is told (``pre``), what a fresh handle
is told (``full``), the run (``run``, a verb of test_handle_reuse_gpu.execute) and the oracle's value of the step.  It
needs no device: the oracle, numpy and the library's host-only queries.  Inputs come from helpers, lds_cases,
stream_cases and dm_batch_cases.

A call is a tuple (method of VQEEngine, *args); a circuit is a Circ (the GPU test turns it into a tq.Circuit).

The evaluation counter (include/vqe_hip.h, vqe_set_noise): 0 after set_noise; + 1 per energy or state run; + maxfun + 1
per COBYLA run; unchanged by exact-mode runs, gradient and L-BFGS runs, reductions and refused calls.  Walk keeps it, and
the oracle's draws of a noisy step are those of noise_draws(seed, stream, counter, ...).  A noisy step is replayed on a
fresh handle only where the counter is 0 (a fresh handle starts there)."""
import collections
import functools

import numpy as np

import lbfgs_helpers as lh
import vqe_oracle as vo
from dm_batch_cases import noisy as dm_noisy
from helpers import fermionic_hamiltonian, random_gates, random_hamiltonian, random_state, shift_grad
from lds_cases import A_TOL, E_TOL, cobyla_circuit, inputs
from lds_cases import energy_of as _energy_of, run_circuit as _run_circuit

G_TOL = 1e-10            # gradients: times max(1, sum |c_k|), the bound of tests/test_grad_gpu.py
LOOSE_TOL = 1e-12        # a step whose cached plan may order a sum differently (tests/test_engine_plumbing's bound)
DISTINCT = 1e-6          # consecutive expected values of one shape differ by more than this (test_handle_reuse_cpu)
VQE_EINVAL, VQE_ESTATE = -22, -1
LBFGS = dict(history=3, maxiter=4, maxfun=40)

Circ = collections.namedtuple("Circ", "kind q0 q1 pidx P")
# scenario -> seed, where seed 0 did not give distinct consecutive steps (test_handle_reuse_cpu finds the first that does
# and fails until it is recorded here; none so far)
SEEDS = {}


def circ_of(gates, P):
    return Circ(*(np.asarray(a, np.int32) for a in gates[:4]), int(P))


EMPTY = circ_of(tuple(np.zeros(0, np.int32) for _ in range(4)), 0)


def co():
    import c_oracle
    return c_oracle


def term_owner(n, xmask, world):
    """vqe_term_owner (host only)"""
    from tensorrl_qas_amd import parallel
    return np.asarray(parallel.term_owner(n, np.ascontiguousarray(xmask, np.uint64), world))


def scale_of(ham):
    return max(1.0, float(np.abs(ham[2]).sum()))


def pre_action(c, theta, new_gate):
    """The circuit the optimiser of an environment step sees (pre_action, csrc/vqe_geo.h): lbfgs_helpers.pre_action on a
    Circ, and the channel that construct_ansatz attached to the new gate - a DEPOL1 right behind a rotation on its
    qubit, a DEPOL2 right behind a CNOT on its qubits - leaves with it.  -> (Circ, x0, hole)"""
    g, x0, hole = lh.pre_action(c.kind, c.q0, c.q1, c.pidx, theta, new_gate)
    if 0 <= new_gate < len(c.kind) - 1:
        k, f = int(c.kind[new_gate]), new_gate + 1
        if (c.kind[f] == 4 and k in (1, 2, 3) and c.q0[f] == c.q0[new_gate]) or \
                (c.kind[f] == 5 and k == 0 and c.q0[f] == c.q0[new_gate] and c.q1[f] == c.q1[new_gate]):
            keep = np.arange(len(g[0])) != new_gate      # (the follower sits at the new gate's place now)
            g = tuple(a[keep] for a in g)
    return circ_of(g, x0.size), x0, hole


Step = collections.namedtuple("Step", "label pre full run expect post fresh fp same_as loose repeat layout info")


class Walk:
    """Builds one scenario.  do(): a setter on the reused handle (and in the configuration a fresh handle gets);
    step(): a run.  The configuration is kept so that ``full`` can be written out at every step."""

    def __init__(self, name, n, psi, ham, fingerprints=True):
        self.name, self.n = name, n
        self.fingerprints = fingerprints      # False: no walks of the host optimisers (``fp``, read by the CPU test only)
        self.psi, self.ham = None, None
        self.shard, self.noise_calls, self.mode, self.dmb = (0, 1), [], 0, None
        self.flags, self.trace, self.circ, self.batch, self.new_gate = {}, False, None, None, None
        self.p1 = self.p2 = self.sigma = 0.0
        self.seed = 0
        self.counter = 0
        self.pending, self.steps, self.checks = [], [], []
        self.do("set_init_state", psi)
        self.do("set_hamiltonian", *ham)

    # ---- setters ----------------------------------------------------------------------------------------------------
    def do(self, method, *args):
        self.pending.append((method,) + args)
        if method in ("set_init_state", "set_init_state_from_device"):
            self.psi_call, self.psi = (method, args[0]), args[0]
        elif method == "set_hamiltonian":
            self.ham = tuple(args)
        elif method == "set_term_shard":
            self.shard = tuple(args)
        elif method == "set_noise":
            self.p1, self.p2, self.seed = args
            self.counter = 0
            self._noise_call(method, args)
        elif method == "set_shot_noise":
            self.sigma, self.seed = args
            self._noise_call(method, args)
        elif method == "set_noise_mode":
            self.mode = args[0]
        elif method == "set_dm_batched":
            self.dmb = args[0]
        elif method in ("set_stream_grad", "set_stream_lbfgs"):
            self.flags[method] = args[0]
        elif method == "batch_set_trace":
            self.trace = args[0]
        elif method == "set_circuit":
            self.circ = args[0]
        elif method == "batch_load":
            self.batch, self.new_gate = (list(args[0]), [np.asarray(t, np.float64) for t in args[1]]), None
        elif method == "batch_set_new_gate":
            self.new_gate = None if args[0] is None else np.asarray(args[0], np.int32)
        else:
            raise KeyError(method)

    def _noise_call(self, method, args):      # the two calls in the order they were made last: the later one sets the seed
        self.noise_calls = [c for c in self.noise_calls if c[0] != method] + [(method,) + tuple(args)]

    def full(self, batch):
        """what a fresh handle is told to be in this configuration (``batch``: the run works on the resident batch)"""
        out = [self.psi_call, ("set_hamiltonian",) + self.ham]
        if self.shard != (0, 1):
            out.append(("set_term_shard",) + self.shard)
        out += self.noise_calls
        if self.mode:
            out.append(("set_noise_mode", self.mode))
        if self.dmb is not None:
            out.append(("set_dm_batched", self.dmb))
        out += [(k, v) for k, v in sorted(self.flags.items())]
        if self.trace:
            out.append(("batch_set_trace", True))
        if batch:
            out.append(("batch_load",) + self.batch)
            if self.new_gate is not None:
                out.append(("batch_set_new_gate", self.new_gate))
        elif self.circ is not None:
            out.append(("set_circuit", self.circ))
        return out

    # ---- the oracle in this configuration ---------------------------------------------------------------------------
    def my_ham(self):
        r, w = self.shard
        if w == 1 or self.ham[0].size == 0:
            return self.ham
        keep = term_owner(self.n, self.ham[0], w) == r
        return tuple(a[keep] for a in self.ham)

    def psi0(self):
        if self.psi is None:
            v = np.zeros(1 << self.n, np.complex128)
            v[0] = 1.0
            return v
        return self.psi

    def noisy(self):
        return self.mode == 0 and (self.p1 > 0 or self.p2 > 0 or self.sigma > 0)

    def state(self, c, th, stream=0, counter=None, fast=False):
        dr = None
        if self.mode == 0 and (self.p1 > 0 or self.p2 > 0):
            dr = co().noise_draws(self.seed, stream, self.counter if counter is None else counter, c.kind, self.p1, self.p2)
        if fast:
            return co().run_circuit(self.n, self.psi0(), c.kind, c.q0, c.q1, c.pidx, th, dr)
        return _run_circuit(self.n, self.psi0(), c.kind, c.q0, c.q1, c.pidx, th, dr)

    def energy(self, c, th, stream=0, counter=None, fast=False):
        """the oracle's energy of circuit c at th as evaluation ``counter`` of stream ``stream`` (fast: the C oracle at
        every size - for the fingerprints of the CPU test, not for a comparison with the device)"""
        ham = self.my_ham()
        th = np.asarray(th, np.float64)
        if self.mode == 1:
            return float(vo.energy_dm(vo.run_circuit_dm(self.psi0(), c.kind, c.q0, c.q1, c.pidx, th, self.p1, self.p2), *ham)) \
                if ham[0].size else 0.0
        psi = self.state(c, th, stream, counter, fast)
        e = 0.0
        if ham[0].size:
            e = co().energy_pauli(self.n, psi, *ham) if fast else _energy_of(self.n, psi, ham)
        if self.sigma > 0:
            e += self.sigma * co().lib().orc_noise_gauss(self.seed, stream, self.counter if counter is None else counter)
        return float(e)

    def grad(self, c, th):
        ham = self.my_ham()
        if not ham[0].size:
            return np.zeros(c.P)
        n = self.n
        return shift_grad(self.psi0(), c.kind, c.q0, c.q1, c.pidx, np.asarray(th, np.float64), ham,
                          energy=lambda p, k, a, b, pi, t, h: _energy_of(n, _run_circuit(n, p, k, a, b, pi, t), h))

    def host_cobyla(self, c, x0, maxfun):
        """(x, f, nfev) of the library's host COBYLA on the oracle's clean objective (a fingerprint: what the device
        should find)"""
        import tensorrl_qas_amd as tq
        if not self.fingerprints:
            return None, None, None
        if c.P == 0:
            return np.zeros(0), self.energy(c, x0, fast=True), 1
        return tq.HostCobyla(x0, 1.0, 1e-4, maxfun).minimize(lambda x: self.energy(c, x, fast=True))[:3]

    def host_lbfgs(self, c, x0, opts):
        ham = self.my_ham()
        if not self.fingerprints:
            return None, None, None
        if c.P == 0 or not ham[0].size:      # (no parameter, or E = 0 everywhere: the gradient test stops at x0)
            return np.array(x0, np.float64), self.energy(c, x0, fast=True), 1
        r = lh.lbfgs(lh.oracle_fun(self.psi0(), c.kind, c.q0, c.q1, c.pidx, c.P, ham), x0, scale=scale_of(ham), **opts)
        return r.x, r.f, r.nfev

    def optimiser_fp(self, env_step, optimise):
        """the expected f of an optimiser run on the resident batch: optimise(Circ, x0) -> (x, f) on the circuits the
        optimiser sees; an env-step merges the optimum into theta0 (the new gate keeps its angle), rounds to float32 and
        evaluates the full circuit"""
        cs, ths = self.batch
        out = []
        if not self.fingerprints:
            return None
        for (c, th), (sub, x0, hole) in zip(zip(cs, ths), self._optimised(env_step)):
            x, f = optimise(sub, x0)[:2]
            if env_step:
                full = np.array(th, np.float64)
                full[[j for j in range(c.P) if j != hole]] = x
                f = self.energy(c, full.astype(np.float32).astype(np.float64), fast=True)
            out.append(f)
        return np.array(out)

    # ---- runs -------------------------------------------------------------------------------------------------------
    def _add(self, label, run, batch, expect, post, fp, fresh=None, same_as=None, loose=None, repeat=False, layout=None,
             info=None):
        if fresh is None:
            fresh = not self.noisy() or self.counter == 0
        self.steps.append(Step(f"{len(self.steps)}:{label}", self.pending, self.full(batch), run, expect, post, fresh,
                               None if fp is None else np.atleast_1d(np.asarray(fp, np.float64)), same_as, loose, repeat,
                               layout, info))
        self.pending = []
        return len(self.steps) - 1

    def _bump(self, optimiser_maxfun=None, state=False):
        if self.mode == 1 and not state:      # (vqe_get_state has no exact-channel form: it counts in mode 1 too)
            return
        self.counter += 1 if optimiser_maxfun is None else optimiser_maxfun + 1

    def energy_batch(self, thetas, **kw):
        thetas = np.asarray(thetas, np.float64).reshape(-1, self.circ.P)
        ref = np.array([self.energy(self.circ, t, b) for b, t in enumerate(thetas)])
        i = self._add("energy_batch", ("energy_batch", thetas), False, {"e": (ref, E_TOL)}, None, ref, **kw)
        self._bump()
        return i

    def get_state(self, theta, **kw):
        ref = self.state(self.circ, theta)
        i = self._add("get_state", ("get_state", np.asarray(theta, np.float64)), False, {"psi": (ref, A_TOL)}, None,
                      np.concatenate([ref.real, ref.imag]), **kw)
        self._bump(state=True)
        return i

    def energy_grad(self, theta, **kw):
        e, g = self.energy(self.circ, theta), self.grad(self.circ, theta)
        return self._add("energy_grad", ("energy_grad", np.asarray(theta, np.float64)), False,
                         {"e": (np.array([e]), E_TOL * scale_of(self.my_ham())), "g": (g, G_TOL * scale_of(self.my_ham()))},
                         None, np.concatenate([[e], g]), **kw)

    def _at_optimum(self, circuits, starts=None):
        """post check of an optimiser run: f is the oracle's energy at the x the device returned; ``starts`` (the x0 of a
        run that is no env-step): the optimiser returns its best point, so f is not above the oracle's E(x0), and a run
        on a circuit with parameters and a Hamiltonian with terms made more than the one evaluation of x0 - two handles
        that both hand x0 back do not pass"""
        snap = _Frozen(self)
        has_terms = bool(self.my_ham()[0].size)

        def post(res):
            worst = 0.0
            x = res["x"]
            off = 0
            for b, c in enumerate(circuits):
                f = float(np.atleast_1d(res["f"])[b])
                worst = max(worst, abs(f - snap.energy(c, x[off:off + c.P])))
                if starts is not None:
                    assert f <= snap.energy(c, starts[b]) + E_TOL, (b, f)
                    assert int(np.atleast_1d(res["nfev"])[b]) > 1 or not (c.P and has_terms), b
                off += c.P
            assert worst < E_TOL, worst
            return worst
        return post

    def minimize_cobyla(self, x0, maxfun, **kw):
        assert maxfun <= self.circ.P + 12 and not self.noisy()
        fp = self.host_cobyla(self.circ, x0, maxfun)[1:]      # (f, nfev): what a one-circuit optimiser run returns beside x
        i = self._add("minimize_cobyla", ("minimize_cobyla", np.asarray(x0, np.float64), maxfun), False, {},
                      self._at_optimum([self.circ], [x0]), fp if self.fingerprints else None, **kw)
        self._bump(maxfun)
        return i

    def minimize_lbfgs(self, x0, **kw):
        fp = self.host_lbfgs(self.circ, x0, LBFGS)[1:]
        post = self._at_optimum([self.circ], [x0])
        if not self.my_ham()[0].size:      # no term at all: E = 0 and g = 0 at x0, the first test (max |g| <= gtol) stops there
            x0c, at = np.array(x0, np.float64), post

            def post(res):
                assert res["f"][0] == 0.0 and np.array_equal(res["x"], x0c), res
                assert (int(res["nfev"][0]), int(res["nit"][0]), int(res["status"][0])) == (1, 0, 0), res
                return at(res)
        return self._add("minimize_lbfgs", ("minimize_lbfgs", np.asarray(x0, np.float64), LBFGS), False, {},
                         post, fp if self.fingerprints else None, **kw)

    def batch_energy(self, **kw):
        cs, ths = self.batch
        ref = np.array([self.energy(c, t, b) for b, (c, t) in enumerate(zip(cs, ths))])
        i = self._add("batch_run_energy", ("batch_run_energy",), True, {"f": (ref, E_TOL)}, None, ref, **kw)
        self._bump()
        return i

    def batch_reduction(self, after, why, **kw):
        """vqe_batch_run_reduction on the states step ``after`` left (streaming path): that step's f again, at LOOSE_TOL -
        the reduction-only launch plans energy passes of its own (``why``: the line), the run before summed inside its
        last circuit pass"""
        return self._add("batch_run_reduction", ("batch_run_reduction",), True, {}, None, self.steps[after].fp, fresh=False,
                         same_as=after, loose=why, **kw)

    def fetch_only(self, after, traced=(), lbfgs=False, **kw):
        """the results of step ``after`` are still there (traced: and the traces of these circuits; lbfgs: and nit / status)"""
        return self._add("fetch", ("fetch", tuple((b, self.batch[0][b].P) for b in traced), lbfgs), True, {}, None, self.steps[after].fp, fresh=False,
                         same_as=after, **kw)

    def batch_grad(self, **kw):
        cs, ths = self.batch
        e = np.array([self.energy(c, t) for c, t in zip(cs, ths)])
        g = np.concatenate([self.grad(c, t) for c, t in zip(cs, ths)] + [np.zeros(0)])
        s = scale_of(self.my_ham())
        return self._add("batch_run_energy_grad", ("batch_run_energy_grad",), True, {"f": (e, E_TOL * s), "g": (g, G_TOL * s)},
                         None, np.concatenate([e, g]), **kw)

    def _optimised(self, env_step):
        """[(Circ the optimiser sees, x0, hole)] of the resident batch"""
        cs, ths = self.batch
        ng = self.new_gate if (env_step and self.new_gate is not None) else np.full(len(cs), -1)
        return [pre_action(c, t, int(g)) for c, t, g in zip(cs, ths, ng)]

    def batch_minimize(self, maxfun, env_step=False, traced=(), fingerprint=True, **kw):
        cs, ths = self.batch
        assert maxfun <= max(c.P for c in cs) + 12
        fp = None
        if fingerprint and not self.noisy():
            fp = self.optimiser_fp(env_step, lambda c, x0: self.host_cobyla(c, x0, maxfun))
        elif fingerprint and self.fingerprints and self.mode == 0:      # evaluation k of stream b under the draws of counter + k
            import tensorrl_qas_amd as tq
            fp = []
            for b, ((c, th), (sub, x0, hole)) in enumerate(zip(zip(cs, ths), self._optimised(env_step))):
                k = [self.counter]

                def fun(x, b=b, sub=sub, k=k):
                    k[0] += 1
                    return self.energy(sub, x, b, k[0], fast=True)
                x, f = tq.HostCobyla(x0, 1.0, 1e-4, maxfun).minimize(fun)[:2] if sub.P else (x0, fun(x0))
                if env_step:      # the full circuit at the rounded angles, drawn at counter + maxfun + 1
                    full = np.array(th, np.float64)
                    full[[j for j in range(c.P) if j != hole]] = x
                    f = self.energy(c, full.astype(np.float32).astype(np.float64), b, self.counter + maxfun + 1, fast=True)
                fp.append(f)
        if not self.noisy():
            post = self._at_optimum(cs, None if env_step else ths)
        elif env_step:
            post = self._noisy_env_step(cs, maxfun)
        else:
            post = None
        if traced:
            post = self._trace_check(cs, traced, env_step, post)
        verb = "batch_run_env_step" if env_step else "batch_run_minimize"
        if isinstance(kw.get("info"), dict):      # batched exact mode: lock-step evaluations = the largest nfev (+ the full circuits)
            kw["info"] = dict(kw["info"], evaluations="nfev+1" if env_step else "nfev")
        i = self._add(verb, (verb, maxfun, tuple((b, cs[b].P) for b in traced)), True, {}, post, fp, **kw)
        self._bump(maxfun)
        return i

    def _noisy_env_step(self, cs, maxfun):
        """f of a noisy env-step: the FULL circuit at the x the device returned, under the draws of evaluation
        counter + maxfun + 1 numbered by gate position in the full circuit (include/vqe_hip.h, vqe_set_noise)"""
        snap = _Frozen(self)

        def post(res):
            worst, off = 0.0, 0
            for b, c in enumerate(cs):
                worst = max(worst, abs(res["f"][b] - snap.energy(c, res["x"][off:off + c.P], b, snap.counter + maxfun + 1)))
                off += c.P
            assert worst < E_TOL, worst
            return worst
        return post

    def _trace_check(self, cs, traced, env_step, then):
        """every traced value is the oracle's energy at the traced point - under the draws of evaluation counter + k"""
        snap, seen, base = _Frozen(self), self._optimised(env_step), self.counter

        def post(res):
            worst = then(res) if then else 0.0
            for b in traced:
                c = seen[b][0]
                ft, xt = res[f"trace{b}"]
                assert not np.any(xt[:, c.P:])      # (an env-step whose new gate is a rotation optimises one variable less)
                xt = xt[:, :c.P]
                nfev = int(res["nfev"][b])
                assert nfev >= 1 and np.array_equal(xt[0], seen[b][1])
                for k in range(nfev):
                    worst = max(worst, abs(ft[k] - snap.energy(c, xt[k], b, base + k + 1)))
                assert not np.any(ft[nfev:]) and not np.any(xt[nfev:])      # zero beyond nfev: no stale rows
                if not env_step:      # what was published is one of the evaluations: its point, and the value it had there
                    off = sum(q.P for q in cs[:b])
                    x = res["x"][off:off + c.P]
                    k = int(np.argmin([np.abs(xt[j] - x).max() for j in range(nfev)]))
                    assert np.abs(xt[k] - x).max() <= 1e-12 and res["f"][b] == ft[k], (b, k, res["f"][b], ft[k])
                    assert np.array_equal(res["xopt"][off:off + c.P], x), b
            assert worst < E_TOL, worst
            return worst
        return post

    def batch_lbfgs(self, env_step=False, opts=LBFGS, **kw):
        cs, ths = self.batch
        fp = self.optimiser_fp(env_step, lambda c, x0: self.host_lbfgs(c, x0, opts))
        verb = "batch_run_env_step_lbfgs" if env_step else "batch_run_minimize_lbfgs"
        return self._add(verb, (verb, opts), True, {}, self._at_optimum(cs), fp, **kw)

    def refused(self, code, method, *args, **kw):
        """a call that must fail with ``code`` and leave the handle as it was (the steps after it say whether it did)"""
        self.pending.append(("refused", code, method) + args)

    def same_bits(self, i, j):
        self.checks.append(("same_bits", i, j))

    def sums_to(self, steps, key, ref, tol):
        self.checks.append(("sum", tuple(steps), key, np.asarray(ref), tol))


class _Frozen:
    """the oracle of a Walk as it was configured when a step was made (post checks run later)"""

    def __init__(self, w):
        self.__dict__.update({k: getattr(w, k) for k in ("n", "psi", "ham", "shard", "mode", "p1", "p2", "sigma", "seed", "counter")})

    my_ham, psi0, state, energy = Walk.my_ham, Walk.psi0, Walk.state, Walk.energy


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _gates(n, G, rng, p_cnot=0.35):
    k, a, b, p, th = random_gates(n, G, rng, p_cnot=p_cnot if n > 1 else 0.0)
    return circ_of((k, a, b, p), th.size), th


def _tie_free(n, P, seed):
    g, th = cobyla_circuit(n, P, seed)
    return circ_of(g, P), th


def hamiltonian_walk(n, rng):
    """S1: [(name, ham, layout class)]"""
    ferm = fermionic_hamiltonian(n, n_hop=n, n_quad=n // 2, rng=rng, dressed=1)
    cplx = random_hamiltonian(n, 6 + 2 * n, rng, real=False)
    cplx = tuple(a[cplx[0] != 0] for a in cplx)                                        # no diagonal group
    assert any(bin(int(x & z)).count("1") % 2 for x, z in zip(cplx[0], cplx[1]))       # an imaginary section
    z = rng.integers(1, 1 << n, 2 * n).astype(np.uint64)
    diag = (np.zeros(z.size, np.uint64), z, rng.normal(size=z.size))
    zero = (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    return [("fermionic", ferm, "units"), ("complex", cplx, "no_units"), ("diagonal", diag, "diag_only"), ("zero", zero, "empty"),
            ("fermionic again", ferm, "units")]


# ---- S1: Hamiltonian walk on the LDS path -----------------------------------------------------------------------------
def s1(n, seed=0, fp=True):
    rng = np.random.default_rng(9100 + n + 1000 * seed)
    psi = random_state(n, rng)
    hams = hamiltonian_walk(n, rng)
    c, th = _tie_free(n, 8, 9150 + n + 1000 * seed)
    thetas = np.stack([th, th + 0.3, -th])
    w = Walk(f"S1 n={n}", n, psi, hams[0][1], fingerprints=fp)
    w.do("set_circuit", c)
    first = None
    for k, (name, ham, layout) in enumerate(hams):
        if k:
            w.do("set_hamiltonian", *ham)
        back = k == len(hams) - 1      # the first Hamiltonian again, at the first angles: the bits of the first stop
        same = (lambda i: first[i]) if back else (lambda i: None)
        d = 0.0 if back else 0.1 * k
        ids = [w.energy_batch(thetas + d, layout=layout, same_as=same(0)), w.get_state(th + d, same_as=same(1)),
               w.energy_grad(th + d, same_as=same(2)), w.minimize_cobyla(th + d, c.P + 10, same_as=same(3)),
               # (at the zero-term stop both optimisers expect f = 0; they differ in nfev: the L-BFGS stops at x0)
               w.minimize_lbfgs(th + d, same_as=same(4))]
        first = first or ids
    for i, j in zip(first, ids):
        w.same_bits(i, j)
    return w


# ---- S2: term-shard walk ----------------------------------------------------------------------------------------------
def s2(n, seed=0, fp=True):
    rng = np.random.default_rng(9200 + n + 1000 * seed)
    psi, ham = inputs(n)
    c, th = _gates(n, 24, rng)
    w = Walk(f"S2 n={n}", n, psi, ham, fingerprints=fp)
    w.do("set_circuit", c)
    at = {}
    for k, (r, world) in enumerate([(0, 1), (1, 3), (2, 3), (0, 3), (0, 2), (0, 1)]):
        if k:
            w.do("set_term_shard", r, world)
        last = k == 5
        e = w.energy_batch(np.stack([th, 0.5 * th]), same_as=0 if last else None)
        g = w.energy_grad(th, same_as=1 if last else None)
        at[(r, world, k)] = (e, g)
        if world > 1:      # refused while sharded; the next energy has the bits of the one before
            w.refused(VQE_ESTATE, "minimize_cobyla", th, 1.0, 1e-4, 10)
            w.refused(VQE_ESTATE, "minimize_lbfgs", th)
            w.energy_batch(np.stack([th, 0.5 * th]), same_as=e)
    w.ham, w.shard = ham, (0, 1)
    full_e = np.array([w.energy(c, th), w.energy(c, 0.5 * th)])
    full_g = np.concatenate([[full_e[0]], w.grad(c, th)])
    thirds = [v for (r, world, k), v in at.items() if world == 3]
    w.sums_to([v[0] for v in thirds], "e", full_e, 3 * E_TOL)
    w.sums_to([v[1] for v in thirds], "eg", full_g, 3 * G_TOL * scale_of(ham))
    w.same_bits(at[(0, 1, 0)][0], at[(0, 1, 5)][0])
    w.same_bits(at[(0, 1, 0)][1], at[(0, 1, 5)][1])
    return w


# ---- S3: batch-shape walk, the VecCircuitEnv pattern ------------------------------------------------------------------
S3_SHAPES = ((0, 1, 24), (25, 33, 64, 8, 0, 40, 12), (70,), (64, 33, 25, 3, 40, 0, 17), (2, 9, 0, 5, 13))
S3_SIZES = (3, 70, 1, 70, 5)


def s3_batches(n, seed=0):
    """-> [([Circ], [theta], new_gate)] of the five batches: parameter counts S3_SHAPES in turn, CNOTs in between"""
    out = []
    for k, (B, shape) in enumerate(zip(S3_SIZES, S3_SHAPES)):
        cs, ths, ng = [], [], []
        for b in range(B):
            P = shape[b % len(shape)]
            if P:
                c, th = _tie_free(n, P, 9300 + 1000 * seed + 100 * k + b + 7 * n)
            else:      # no parameters: CNOTs only, or no gate at all
                c, th = (EMPTY, np.zeros(0)) if b % 2 == 0 or n < 2 else (circ_of(random_gates(n, 4, np.random.default_rng(b), p_cnot=1.0), 0), np.zeros(0))
            cs.append(c), ths.append(th)
            ng.append(len(c.kind) - 1 if len(c.kind) and b % 3 != 2 else -1)      # the gate the action just added: the last one
        out.append((cs, ths, np.array(ng, np.int32)))
    return out


def s3(n, seed=0, fp=True):
    psi, ham = inputs(n)
    w = Walk(f"S3 n={n}", n, psi, ham, fingerprints=fp)
    for k, (cs, ths, ng) in enumerate(s3_batches(n, seed)):
        w.do("batch_load", cs, ths)
        w.batch_energy()
        w.do("batch_set_new_gate", ng)
        mf = max(c.P for c in cs) + 11
        w.batch_minimize(mf, env_step=True)
        w.do("batch_set_trace", True)
        par = [b for b, c in enumerate(cs) if c.P]      # (a circuit without parameters is evaluated once, untraced)
        w.batch_minimize(mf, traced=tuple(sorted({par[0], par[-1]})), info=("placement", int(np.argmax([c.P for c in cs]))))
        w.do("batch_set_trace", False)
    return w


# ---- S4: run kinds interleaved on one resident batch ------------------------------------------------------------------
def s4(n, seed=0, fp=True):
    psi, ham = inputs(n)
    cs, ths = zip(*[_tie_free(n, P, 9450 + n + P + 1000 * seed) for P in (6, 9, 3, 11)])
    cs, ths = list(cs), list(ths)
    ng = np.array([len(cs[0].kind) - 1, 0, -1, len(cs[3].kind) // 2], np.int32)
    w = Walk(f"S4 n={n}", n, psi, ham, fingerprints=fp)
    w.do("batch_load", cs, ths)
    e0 = w.batch_energy(repeat=True)
    w.do("batch_set_new_gate", ng)
    w.batch_minimize(16, env_step=True, repeat=True)
    w.batch_energy(same_as=e0, repeat=True)
    w.batch_lbfgs(repeat=True)
    w.batch_grad(repeat=True)
    w.batch_minimize(18, repeat=True)
    st = w.batch_lbfgs(env_step=True, repeat=True)
    w.batch_energy(same_as=e0)
    w.do("batch_set_new_gate", None)      # cleared: the env-step optimises the full circuits
    w.batch_lbfgs(env_step=True, opts=dict(LBFGS, maxiter=2))      # (other options than the minimise run above: other values)
    w.do("batch_set_new_gate", ng)
    w.batch_lbfgs(env_step=True, same_as=st)
    cs2, ths2 = zip(*[_tie_free(n, P, 9470 + n + P + 1000 * seed) for P in (6, 9, 3, 11)])
    w.do("batch_load", list(cs2), list(ths2))      # a load clears the new gates
    w.batch_minimize(16, env_step=True)
    # a one-circuit energy in between replaces the resident batch (include/vqe_hip.h, vqe_batch_load)
    w.do("set_circuit", cs[1])
    w.energy_batch(ths[1][None, :] + 0.25)
    w.do("batch_load", list(cs2), list(ths2))
    w.batch_energy()
    return w


# ---- S5: noise switches -----------------------------------------------------------------------------------------------
SEED_A, SEED_B = 20240607, 977
S5_P = (0.25, 0.5)


def s5(n, seed=0, fp=True):
    rng = np.random.default_rng(9500 + n + 1000 * seed)
    psi, ham = inputs(n)
    base = random_gates(n, 7 if n >= 10 else 9, rng)
    while base[4].size < 3:
        base = random_gates(n, 7 if n >= 10 else 9, rng)
    g = dm_noisy(base)
    c, th = circ_of(g, base[4].size), base[4]
    thetas = np.stack([th, th + 0.4, 0.5 * th])
    b2 = dm_noisy(random_gates(n, 5, rng, p_cnot=0.3))
    small = [(c, th), (circ_of(b2, b2[4].size), b2[4])]
    w = Walk(f"S5 n={n}", n, psi, ham, fingerprints=fp)
    w.do("set_circuit", c)
    clean = w.energy_batch(thetas)
    w.do("set_noise", *S5_P, SEED_A)
    w.energy_batch(thetas)                       # counter 0: also against a fresh handle
    w.energy_batch(thetas)                       # counter 1
    w.do("batch_set_trace", True)
    w.do("batch_load", [s[0] for s in small], [s[1] for s in small])
    mf = max(s[0].P for s in small) + 6
    w.batch_minimize(mf, traced=(0, 1))      # evaluations counter + 1 ...
    w.do("batch_set_trace", False)
    w.do("batch_set_new_gate", np.array([max(k for k in range(len(s[0].kind)) if s[0].kind[k] < 4) for s in small], np.int32))
    w.batch_minimize(mf, env_step=True)      # its last evaluation, of the full circuits, at counter + maxfun + 1
    w.do("set_noise_mode", 1)
    ex_c, ex_th = c, thetas
    if n >= 10:      # (the numpy channel oracle takes a third of a second per noise gate on 2^20 entries)
        short = dm_noisy(random_gates(n, 3, rng, p_cnot=0.3))
        ex_c, ex_th = circ_of(short, short[4].size), np.stack([short[4], short[4] + 0.4, 0.5 * short[4]])
        w.do("set_circuit", ex_c)
    serial = w.energy_batch(ex_th, info="serial")
    w.do("set_dm_batched", 2)
    w.energy_batch(ex_th + 0.2, info=dict(resident=2, chunks=2, evaluations=1))      # (other angles: the serial values would not do)
    w.do("set_dm_batched", 0)
    w.energy_batch(ex_th, same_as=serial, info="serial")
    w.do("set_noise_mode", 0)
    w.do("set_circuit", c)
    assert w.counter == 2 + 2 * (mf + 1)
    w.energy_batch(thetas)                       # trajectories go on where they stopped
    w.do("set_noise", 0.0, 0.0, SEED_A)
    w.energy_batch(thetas, same_as=clean)
    w.do("set_shot_noise", 0.37, SEED_A)
    w.energy_batch(thetas)                       # counter 1 (set_noise made it 0, the clean run 1): not restarted
    w.do("set_shot_noise", 0.0, SEED_A)
    w.energy_batch(thetas, same_as=clean)
    # one seed per handle, the later call sets it; only set_noise restarts the counter
    w.do("set_noise", *S5_P, SEED_A)
    w.do("set_shot_noise", 0.37, SEED_B)
    w.energy_batch(thetas)                       # counter 0, Pauli draws and shot draws of SEED_B
    w.energy_batch(thetas)
    w.do("set_shot_noise", 0.21, SEED_B)
    w.do("set_noise", *S5_P, SEED_A)
    w.energy_batch(thetas)                       # counter 0, both of SEED_A
    w.do("set_shot_noise", 0.21, SEED_B)         # counter stays 1
    w.energy_batch(thetas)
    return w


# ---- S6: exact channel mode, both forms -------------------------------------------------------------------------------
def s6_batches(n, seed=0):
    """-> (circuits of dm_batch_cases.mixed_batch - a channel behind every gate, one empty, one clean -, two theta sets,
    two new-gate arrays that differ in every circuit that has two gates)"""
    from dm_batch_cases import mixed_batch
    rng = np.random.default_rng(9600 + n + 1000 * seed)
    raw = mixed_batch(n, 9, rng)
    cs = [circ_of(c, c[4].size) for c in raw]
    th_a = [c[4] for c in raw]
    th_b = [t + rng.uniform(-0.5, 0.5, t.size) for t in th_a]
    gate = lambda c, which: -1 if not len(c.kind) else [k for k in range(len(c.kind)) if c.kind[k] < 4][which]
    ng1 = np.array([gate(c, -1) for c in cs], np.int32)      # the last gate that is no channel
    ng2 = np.array([gate(c, 0) for c in cs], np.int32)       # the first one
    return cs, th_a, th_b, ng1, ng2


def s6(n, seed=0, fp=True):
    rng = np.random.default_rng(9650 + n + 1000 * seed)
    psi = random_state(n, rng)
    ham1, ham2 = random_hamiltonian(n, 20, rng, real=False), random_hamiltonian(n, 14, rng, real=False)
    cs, th_a, th_b, ng1, ng2 = s6_batches(n, seed)
    B = len(cs)
    mf = max(c.P for c in cs) + 8
    w = Walk(f"S6 n={n}", n, psi, ham1, fingerprints=fp)
    w.do("set_noise", 0.05, 0.2, 5)
    w.do("set_noise_mode", 1)
    w.do("batch_load", cs, th_a)
    serial = w.batch_energy(info="serial")
    w.do("batch_set_new_gate", ng1)
    w.batch_minimize(mf, env_step=True, info="serial")
    w.do("set_dm_batched", 1)
    w.do("batch_load", cs, th_b)
    lock = w.batch_energy(info=dict(resident=1, chunks=B, evaluations=1))
    w.do("set_dm_batched", 2)      # the bits of a circuit do not depend on R (include/vqe_hip.h)
    w.batch_energy(same_as=lock, info=dict(resident=2, chunks=(B + 1) // 2, evaluations=1))
    w.do("set_dm_batched", -1)     # dm_auto_cap is worked out anew
    w.batch_energy(same_as=lock, info=dict(resident=B, chunks=1, evaluations=1))
    w.do("set_dm_batched", 0)
    w.do("batch_load", cs, th_a)
    w.batch_energy(same_as=serial, info="serial")
    w.do("set_dm_batched", -1)
    all_in = dict(resident=B, chunks=1)
    w.do("set_noise", 0.15, 0.02, 5)      # the plan's dep table follows p1 / p2 (no reload)
    w.batch_energy(info=dict(all_in, evaluations=1))
    w.do("set_hamiltonian", *ham2)        # dm_ham_gen
    whole = w.batch_energy(info=dict(all_in, evaluations=1))
    halves = []
    for r in (0, 1):
        w.do("set_term_shard", r, 2)
        halves.append(w.batch_energy(info=dict(all_in, evaluations=1)))
    w.do("set_term_shard", 0, 1)
    w.batch_energy(same_as=whole, info=dict(all_in, evaluations=1))
    w.sums_to(halves, "f", w.steps[whole].expect["f"][0], 2 * E_TOL)
    w.do("batch_load", cs, th_b)          # a second batch of equal shape
    w.batch_energy(info=dict(all_in, evaluations=1))
    w.do("batch_set_new_gate", ng1)       # two env-steps with different new gates and no reload: dmb_pre must follow
    env1 = w.batch_minimize(mf, env_step=True, info=all_in)
    w.do("batch_set_new_gate", ng2)
    w.batch_minimize(mf, env_step=True, info=all_in)
    w.batch_minimize(mf, info=all_in)
    w.do("set_dm_batched", 2)
    w.do("batch_set_new_gate", ng1)      # the first new gates again, in chunks of two: the bits of the first env-step
    last = w.batch_minimize(mf, env_step=True, same_as=env1, info=dict(resident=2, chunks=(B + 1) // 2))
    # a batch of the same shape with an RXX gate: the load is taken, every run refused; the results of the run before
    # are still there, and the next valid batch runs clean
    c0 = cs[0]
    assert c0.P > 0
    rxx = Circ(np.append(c0.kind, 6).astype(np.int32), np.append(c0.q0, 0).astype(np.int32), np.append(c0.q1, 1).astype(np.int32),
               np.append(c0.pidx, 0).astype(np.int32), c0.P)
    w.pending.append(("batch_load", [rxx] + cs[1:], th_b))
    w.refused(VQE_EINVAL, "batch_run_energy")
    w.refused(VQE_EINVAL, "batch_run_env_step", 1.0, 1e-4, mf)
    w.fetch_only(last)
    w.do("batch_load", cs, [t + 0.3 for t in th_a])
    w.batch_energy(info=dict(resident=2, chunks=(B + 1) // 2, evaluations=1))
    return w


# ---- S7: the streaming path, what test_plan_cache leaves out ----------------------------------------------------------
LINE_472 = ("vqe_stream.h:472 - the op plan an energy run cached (k_t_plan_ops WITH the Hamiltonian's groups) serves the "
            "circuit-only call of the gradient; a fresh handle's gradient plans without them, and k_sg_lambda sums over another layout")
LINE_490 = ("vqe_stream.h:490 - an energy behind an op plan cached from a circuit-only call (the gradient's): the energy "
            "passes are planned on passes that were closed without the groups")
LINE_513 = ("vqe_stream.h:513 - the reduction-only launch plans energy passes of its own (plan_energy(false)); the run "
            "before it summed the groups of the last circuit pass inside k_t_ops")


def s7(seed=0, fp=True):
    import stream_cases
    n = 14
    rng = np.random.default_rng(9700 + 1000 * seed)
    psi_a, psi_b = random_state(n, rng), random_state(n, rng)
    ham = stream_cases.H12(n)
    cs, ths = [], []
    for G in (14, 9, 12):
        g = random_gates(n, G, rng, p_cnot=0.4)
        cs.append(circ_of(g, g[4].size)), ths.append(g[4])
    rot = lambda c, which: [k for k in range(len(c.kind)) if c.kind[k] != 0][which]
    ng1 = np.array([rot(cs[0], -1), -1, rot(cs[2], 0)], np.int32)
    ng2 = np.array([rot(cs[0], 0), rot(cs[1], -1), [k for k in range(len(cs[2].kind)) if cs[2].kind[k] == 0][0]], np.int32)
    mf = max(c.P for c in cs) + 6
    w = Walk("S7 n=14", n, psi_a, ham, fingerprints=fp)
    w.do("batch_load", cs, ths)
    e0 = w.batch_energy(repeat=True)
    w.batch_reduction(e0, LINE_513)
    # gradients: opt-in, refused again after opting out; the energy behind them keeps its bits (the energy plan stands)
    w.do("set_stream_grad", True)
    w.batch_grad(loose=LINE_472)
    w.refused(VQE_ESTATE, "batch_run_reduction")      # the gradient's backward sweep undid the circuit
    w.do("set_stream_grad", False)
    w.refused(VQE_EINVAL, "batch_run_energy_grad")
    w.batch_energy(same_as=e0)
    w.batch_reduction(e0, LINE_513)
    # the same for the device L-BFGS.  Its walk amplifies last-place differences of the gradients, so it is compared bit
    # for bit: the batch is loaded again, and both handles plan the circuit-only call without the groups.  The energy
    # behind it then stands on that plan (LINE_490) and has the value, not the bits, of the first one.
    w.do("batch_load", cs, ths)
    w.do("set_stream_lbfgs", True)
    lb = w.batch_lbfgs()
    w.refused(VQE_ESTATE, "batch_run_reduction")
    w.fetch_only(lb, lbfgs=True)      # a refused run gives up nothing: x, f, nfev, nit, status are still there
    w.do("set_stream_lbfgs", False)
    w.refused(VQE_EINVAL, "batch_run_minimize_lbfgs")
    w.batch_energy(same_as=e0, loose=LINE_490)
    w.batch_reduction(e0, LINE_513)
    # two COBYLA env-steps with different new gates and no reload, then the full batch: one gen, two plan_src
    w.do("batch_set_new_gate", ng1)
    w.batch_minimize(mf, env_step=True)
    w.do("batch_set_new_gate", ng2)
    env = w.batch_minimize(mf, env_step=True)
    w.batch_reduction(env, LINE_513)
    w.batch_energy(same_as=e0)
    # another initial state behind cached plans (no gen bump): the resident states must not be reused
    w.do("set_init_state", psi_b)
    eb = w.batch_energy()
    # Pauli noise on (counter 0: a fresh handle draws the same), then off, on a batch with a channel behind every gate
    ncs, nths = [], []
    for G in (7, 5):
        g = dm_noisy(random_gates(n, G, rng, p_cnot=0.4))
        ncs.append(circ_of(g, g[4].size)), nths.append(g[4])
    w.do("batch_load", ncs, nths)
    w.do("set_noise", 0.4, 0.5, SEED_A)
    noisy = w.batch_energy()
    assert any(np.any(co().noise_draws(SEED_A, b, 0, c.kind, 0.4, 0.5)) for b, c in enumerate(ncs))
    w.batch_energy()      # counter 1: against the oracle's draws alone
    w.do("set_noise", 0.0, 0.0, SEED_A)
    w.batch_energy()
    del eb, noisy
    # a circuit-only plan first: reload, gradient (both handles plan without the groups), then the energy behind it
    w.do("batch_load", cs[::-1], ths[::-1])
    w.do("set_stream_grad", True)
    w.batch_grad()
    w.batch_energy(loose=LINE_490)
    return w


# ---- S8: initial states -----------------------------------------------------------------------------------------------
def s8(n, exact=False, seed=0, fp=True):
    rng = np.random.default_rng(9800 + n + 1000 * seed + (50 if exact else 0))
    psi_a, psi_b = random_state(n, rng), random_state(n, rng)
    if n >= 14:
        import stream_cases
        ham = stream_cases.H12(n)
        base = random_gates(n, 12, rng)
    else:
        ham = inputs(n)[1]
        base = random_gates(n, 14, rng)
    if exact:
        base = dm_noisy(base)
    c, th = circ_of(base, base[4].size), base[4]
    w = Walk(f"S8 n={n}{' exact' if exact else ''}", n, psi_a, ham, fingerprints=fp)
    if exact:
        w.do("set_noise", 0.05, 0.1, 3)
        w.do("set_noise_mode", 1)
    w.do("set_circuit", c)
    first = None
    for k, (method, psi) in enumerate([(None, psi_a), ("set_init_state", None), ("set_init_state_from_device", psi_b),
                                       ("set_init_state", psi_a)]):
        if method:
            w.do(method, psi)
        same = (lambda i: first[i]) if k == 3 else (lambda i: None)
        ids = [w.energy_batch(th[None, :], same_as=same(0))] + ([] if exact else [w.get_state(th, same_as=same(1))])
        first = first or ids
    for i, j in zip(first, ids):
        w.same_bits(i, j)
    return w


# ---- S9: refusals leave the handle as it was --------------------------------------------------------------------------
def s9(n, seed=0, fp=True):
    rng = np.random.default_rng(9900 + n + 1000 * seed)
    psi, ham = inputs(n)
    c, th = _tie_free(n, 7, 9950 + n + 1000 * seed)
    w = Walk(f"S9 n={n}", n, psi, ham, fingerprints=fp)
    w.do("set_circuit", c)
    thetas = np.stack([th, 0.7 * th])

    def probe(same=None):
        return [w.energy_batch(thetas, same_as=same and same[0]), w.energy_grad(th, same_as=same and same[1]),
                w.minimize_cobyla(th, c.P + 8, same_as=same and same[2])]
    base = probe()
    # finding 1: a Hamiltonian whose THIRD term uses qubit n is refused; what was grouped before the bad mask must not
    # reach the handle's host copy, from which every later re-shard plans
    bad = random_hamiltonian(n, 9, rng, real=False)
    bad[0][2] |= np.uint64(1 << n)
    w.refused(VQE_EINVAL, "set_hamiltonian", *bad)
    w.pending.append(("expect_terms", int(ham[0].size), int(np.unique(ham[0]).size)))
    probe(base)
    halves = []
    for r, world in ((0, 2), (1, 2)):
        w.do("set_term_shard", r, world)
        halves.append((w.energy_batch(thetas), w.energy_grad(th)))
    w.do("set_term_shard", 0, 1)
    w.pending.append(("expect_terms", int(ham[0].size), int(np.unique(ham[0]).size)))
    probe(base)
    full_e = np.array([w.energy(c, t) for t in thetas])
    w.sums_to([h[0] for h in halves], "e", full_e, 2 * E_TOL)
    w.sums_to([h[1] for h in halves], "eg", np.concatenate([[full_e[0]], w.grad(c, th)]), 2 * G_TOL * scale_of(ham))
    # the other refusals, each followed by the same three runs
    badc = Circ(c.kind, c.q0, c.q1, np.where(c.pidx >= 0, c.pidx + 1, c.pidx).astype(np.int32), c.P)
    w.refused(VQE_EINVAL, "set_circuit", badc)
    probe(base)
    # a resident batch with new gates and a traced env-step behind it; a refused load and refused new gates leave the
    # batch, its new gates and what can be fetched (x, xopt, f, nfev, the traces) as they were
    c2, th2 = _tie_free(n, 5, 9960 + n + 1000 * seed)
    w.do("batch_set_trace", True)
    w.do("batch_load", [c, c2], [th, th2])
    w.do("batch_set_new_gate", np.array([len(c.kind) - 1, 0], np.int32))
    env = w.batch_minimize(c.P + 8, env_step=True, traced=(0, 1))
    w.refused(VQE_EINVAL, "batch_load_flat", np.array([0, 3, 2]), c.kind[:3], c.q0[:3], c.q1[:3], np.full(3, -1), np.array([0, 0, 0]), np.zeros(0))
    w.fetch_only(env, traced=(0, 1))
    w.batch_minimize(c.P + 8, env_step=True, traced=(0, 1), same_as=env)
    w.refused(VQE_EINVAL, "batch_set_new_gate_raw", np.array([len(c.kind), 0], np.int32))
    w.fetch_only(env, traced=(0, 1))
    w.batch_minimize(c.P + 8, env_step=True, traced=(0, 1), same_as=env)
    w.do("batch_set_trace", False)
    w.refused(VQE_ESTATE, "set_amplitude_shard", 0, 2)
    probe(base)
    w.refused(VQE_EINVAL, "set_noise", 1.5, 0.0, 1)
    probe(base)
    # a circuit beyond the LDS op budget: set_circuit takes it, the run is refused; the old circuit set again runs clean
    G = 12000
    huge = Circ(rng.integers(1, 4, G).astype(np.int32), rng.integers(0, n, G).astype(np.int32), np.full(G, -1, np.int32),
                np.arange(G, dtype=np.int32), G)
    w.pending.append(("set_circuit", huge))
    w.refused(VQE_EINVAL, "energy", np.zeros(G))
    w.pending.append(("set_circuit", c))
    probe(base)
    return w


def s9_dense(fp=True):
    """n = 3: a non-Hermitian dense operator is refused"""
    n = 3
    rng = np.random.default_rng(9933)
    psi = random_state(n, rng)
    ham = random_hamiltonian(n, 10, rng, real=False)
    c, th = _tie_free(n, 5, 9934)
    w = Walk("S9 dense n=3", n, psi, ham, fingerprints=fp)
    w.do("set_circuit", c)
    e = w.energy_batch(th[None, :])
    g = w.energy_grad(th)
    m = rng.normal(size=(8, 8)) + 1j * rng.normal(size=(8, 8))
    w.refused(VQE_EINVAL, "set_hamiltonian_dense", m)
    w.pending.append(("expect_terms", int(ham[0].size), int(np.unique(ham[0]).size)))
    w.energy_batch(th[None, :], same_as=e)
    w.energy_grad(th, same_as=g)
    w.do("set_term_shard", 0, 1)
    w.energy_batch(th[None, :], same_as=e)
    return w


# ---- S10: two handles interleaved -------------------------------------------------------------------------------------
def s10(na, nb, seed=0, fp=True):
    """-> two Walks (never told a setter after the first step) whose steps the GPU test runs in strict alternation"""
    out = []
    for k, n in enumerate((na, nb)):
        rng = np.random.default_rng(10000 + 10 * n + k + 1000 * seed)
        psi = random_state(n, rng)
        ham = inputs(n)[1] if k == 0 else random_hamiltonian(n, 6 + 2 * n, rng, real=False)
        c, th = _tie_free(n, 6 + k, 10050 + n + k + 1000 * seed)
        w = Walk(f"S10 {na}+{nb} handle {k} (n={n})", n, psi, ham, fingerprints=fp)
        w.do("set_circuit", c)
        for rep in range(2):
            t = th + 0.2 * rep
            w.energy_batch(np.stack([t, -t]))
            w.energy_grad(t)
            w.minimize_cobyla(t, c.P + 8)
        out.append(w)
    return out


# ---- the table --------------------------------------------------------------------------------------------------------
BUILDERS = {
    "S1-n8": lambda s, fp=True: s1(8, s, fp=fp), "S1-n10": lambda s, fp=True: s1(10, s, fp=fp),
    "S2-n8": lambda s, fp=True: s2(8, s, fp=fp), "S2-n10": lambda s, fp=True: s2(10, s, fp=fp),
    "S3-n4": lambda s, fp=True: s3(4, s, fp=fp), "S3-n10": lambda s, fp=True: s3(10, s, fp=fp),
    "S4-n4": lambda s, fp=True: s4(4, s, fp=fp), "S4-n10": lambda s, fp=True: s4(10, s, fp=fp),
    "S5-n6": lambda s, fp=True: s5(6, s, fp=fp), "S5-n10": lambda s, fp=True: s5(10, s, fp=fp),
    "S6-n4": lambda s, fp=True: s6(4, s, fp=fp), "S6-n5": lambda s, fp=True: s6(5, s, fp=fp),
    "S7-n14": lambda s, fp=True: s7(s, fp=fp),
    "S8-n5": lambda s, fp=True: s8(5, False, s, fp=fp), "S8-n10": lambda s, fp=True: s8(10, False, s, fp=fp),
    "S8-n14": lambda s, fp=True: s8(14, False, s, fp=fp),
    "S8-n4-exact": lambda s, fp=True: s8(4, True, s, fp=fp),
    "S9-n6": lambda s, fp=True: s9(6, s, fp=fp), "S9-n10": lambda s, fp=True: s9(10, s, fp=fp),
    "S9-dense": lambda s, fp=True: s9_dense(fp=fp),
    "S10-10+10a": lambda s, fp=True: s10(10, 10, s, fp=fp)[0], "S10-10+10b": lambda s, fp=True: s10(10, 10, s, fp=fp)[1],
    "S10-4+12a": lambda s, fp=True: s10(4, 12, s, fp=fp)[0], "S10-4+12b": lambda s, fp=True: s10(4, 12, s, fp=fp)[1],
}
NAMES = tuple(BUILDERS)


def min_distance(w):
    """-> (smallest max-norm distance between the expected values of a step and of an EARLIER step of the same shape,
    the pair) over the steps that are not declared to have the same bits (same_as: the GPU test asserts those equal)"""
    best, pair = np.inf, None
    for j, sj in enumerate(w.steps):
        if sj.fp is None:
            continue
        for i in range(j):
            si = w.steps[i]
            if si.fp is None or si.fp.shape != sj.fp.shape or same_root(w, i) == same_root(w, j):
                continue
            d = float(np.abs(si.fp - sj.fp).max())
            if d < best:
                best, pair = d, (si.label, sj.label)
    return best, pair


def same_root(w, i):
    while w.steps[i].same_as is not None:
        i = w.steps[i].same_as
    return i


@functools.lru_cache(maxsize=None)
def scenario(name, fingerprints=True):
    """The scenario of seed SEEDS[name] (0 unless recorded), built once per process and never modified.
    fingerprints=False: without the expected values of the optimiser runs (``fp``), which only the CPU test reads."""
    return BUILDERS[name](SEEDS.get(name, 0), fingerprints)


def first_distinct_seed(name, tries=8):
    """the procedure behind SEEDS: the first seed whose consecutive expected values are distinct"""
    for seed in range(tries):
        d, pair = min_distance(BUILDERS[name](seed))
        if d > DISTINCT:
            return seed
        print(f"{name}: seed {seed} discarded, steps {pair} expect values {d:.2e} apart")
    raise AssertionError(f"{name}: no seed with distinct steps")
