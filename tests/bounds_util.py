"""Asymmetric, per-dimension action bounds inside the optimizer loops: the designed bound sets, the injected draws, the
oracle runs and the comparisons that tests/test_bounds_cpu.py (oracle alone) and tests/test_gpu_optimizer_bounds.py (device
against oracle) share.  Test infrastructure only.

With lo = -hi and the same bounds in every dimension a bound read at the wrong index, a midpoint taken for 0 and a range
taken for 2 * hi all give the right answer; here lo[u] != -hi[u] and (lo[u], hi[u]) differs for every u."""
import numpy as np

from oracle import oracle_np as O
from tests import tail_util as T

F = np.float32
N, H, K, ITERS, A, STEPS = 64, 5, 8, 3, 3, 2
ONE_BELOW = np.nextafter(F(1), F(0))                     # the largest fp32 below 1
# the pendulum sets (U = 1).  narrow: range 0.5 < 2 * 0.3, so SPSA's c_k = 0.3 perturbation leaves the bounds on at least
# one side from ANY solution inside them (spsa.py:70, 76-81)
NARROW = ([0.25], [0.75])
PENDULUM_SETS = {"asym": T.PENDULUM_BOUNDS["asym"], "pos": T.PENDULUM_BOUNDS["pos"], "narrow": NARROW}
SPSA_REACH = 0.6                                         # 2 * c_0: dimensions narrower than this clip both perturbed candidates

SPSA_OUT_OF_REACH = ("asym", "pos")                      # ranges 2.0 and 1.0: no dimension narrower than SPSA_REACH
PSO_Q4_BOTH_SIDES = ("S20-U6-h200",)                     # sets where clip(0) is nearer hi[u] in some dimension (u = 3, 5 of MLP_BOUNDS[6])
LEARNED_CASES = ("S20-U6-h200", "S3-U2-h16")             # test_gpu_control_step_tail.MLP_SHAPES: k_rollout_mlp_q4s / k_rollout_mlp_w4
STATE_SEED = 7

OPTIMIZERS = ("RS", "CEM", "CEM-warm", "PI2", "SPSA", "PSO", "PSO-reset", "CMA", "CMA-pa")


def case_seed(name, opt_name):
    """a fixed seed per (case, optimizer), the same in every process"""
    return sum((i + 1) * ord(c) for i, c in enumerate(name + "/" + opt_name))


def _b(x):
    return np.asarray(x, F).astype(np.float64).reshape(-1)


mlp_bounds = T.mlp_bounds
# the other kernels that form candidates from the bounds (RS, CEM, PI2 each): name -> the problem they run on
KERNEL_CASES = ("S64-U64-h96", "user-U2", "xform-U2", "corr-U2")
CORR_BETA = 1.0                                          # colored-noise exponent of the "corr-U2" mixing matrix (beta > 0)


class XformHandler(O.Handler):
    """oracle handler with next = cur + 0.5 * dev in place of next = cur + dev (system_dynamics_handler.py:148-161):
    the "scaled" inverse target transform of tests/test_gpu_target_transforms.py"""

    def process_output(self, s, raw):
        s, raw = O.f32(s), O.f32(raw)
        dev = (self.mean_t + (raw * (self.std_t + F(1e-7)).astype(F)).astype(F)).astype(F)
        return (s + (F(0.5) * dev).astype(F)).astype(F)


XFORM_SOURCE = """
__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {
    for (int i = 0; i < S; ++i) next[i] = cur[i] + 0.5f * dev[i];
}
"""
_PROBLEMS = {}


def problem(name, num_agents=A):
    """(oracle evaluator, lo, hi, start states [STEPS, A, S], reward name) of a case: ONE source for the CPU and the GPU
    tests, so that what tests/test_bounds_cpu.py asserts about a case's coverage is about the GPU case's inputs"""
    key = (name, num_agents)
    if key not in _PROBLEMS:
        if name in PENDULUM_SETS:
            lo, hi = PENDULUM_SETS[name]
            ev, reward = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True)), "pendulum"
            states = pendulum_states(STEPS, num_agents, STATE_SEED)
        elif name == "user-U2":                          # DYN_USER + REW_USER: a linear model with two inputs, the intended reward
            lo, hi = T.MLP_BOUNDS[2]
            ev, reward = O.Evaluator(T.intended_reward, O.Handler(T.linear_dynamics_np, True)), "user"
            states = pendulum_states(STEPS, num_agents, STATE_SEED)
        else:
            shape = "S3-U2-h16" if name in ("xform-U2", "corr-U2") else name
            dims, acts, S, U, reward = T.MLP_SHAPES[shape]
            lo, hi = mlp_bounds(U)
            ws, bs, stats, ev = T.net(shape, True)
            if name == "xform-U2":
                ev = O.Evaluator(reward, XformHandler(O.MLP(ws, bs, acts), False, True, stats))
            states = T.mlp_states(shape, STEPS, num_agents, STATE_SEED)
        _PROBLEMS[key] = (ev, np.asarray(lo, F), np.asarray(hi, F), states, reward)
    return _PROBLEMS[key]


def case_mix(name, h=H):
    """the [H, H] mixing matrix of a case's draws (None: uncorrelated)"""
    if name != "corr-U2":
        return None
    from blackbox_mpc_amd.utils.colored_noise import colored_noise_mixing
    return np.asarray(colored_noise_mixing(h, CORR_BETA), F)


def pendulum_states(steps, num_agents, seed):
    """[steps, A, 3] near the upright position: the plan that keeps the pendulum there changes sign with the state, so
    the optimizers' means travel towards both bounds"""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-0.6, 0.6, (steps, num_agents))
    return np.stack([np.cos(th), np.sin(th), rng.uniform(-2.0, 2.0, (steps, num_agents))], -1).astype(F)


# ---- comparisons ---------------------------------------------------------------------------------------------------
def check_candidates(got, want, lo, hi, atol, raw=None, what=""):
    """got (the device's candidates [..., U]) against the oracle's `want`: within atol; EXACTLY lo[u] / hi[u] wherever the
    oracle's unclipped value `raw` (default: want, for optimizers that never clip) lies outside the bound by more than atol;
    never outside [lo[u], hi[u]].  Returns per-dimension counts (clipped at hi, clipped at lo, inside), each [U]."""
    lo64, hi64 = _b(lo), _b(hi)
    got64, want64 = np.asarray(got, np.float64), np.asarray(want, np.float64)
    raw64 = want64 if raw is None else np.asarray(raw, np.float64)
    assert got64.shape == want64.shape == raw64.shape and got64.shape[-1] == lo64.shape[0], (what, got64.shape, want64.shape, raw64.shape)
    err = np.abs(got64 - want64)
    assert np.all(err <= atol), "%s: candidates off by %s (atol %s) at %s" % (what, err.max(), atol, np.unravel_index(int(np.argmax(err)), err.shape))
    hi_b, lo_b = np.broadcast_to(hi64, raw64.shape), np.broadcast_to(lo64, raw64.shape)
    at_hi, at_lo = raw64 > hi_b + atol, raw64 < lo_b - atol
    assert np.array_equal(got64[at_hi], hi_b[at_hi]), "%s: clipped candidates must equal hi[u] exactly" % what
    assert np.array_equal(got64[at_lo], lo_b[at_lo]), "%s: clipped candidates must equal lo[u] exactly" % what
    assert np.all(got64 >= lo_b) and np.all(got64 <= hi_b), "%s: candidates outside the bounds" % what
    inside = (raw64 < hi_b - atol) & (raw64 > lo_b + atol)
    ax = tuple(range(raw64.ndim - 1))
    return at_hi.sum(axis=ax), at_lo.sum(axis=ax), inside.sum(axis=ax)


# ---- injected draws --------------------------------------------------------------------------------------------------
def _rademacher(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1.0, 1.0).astype(F)


def edge_uniform(rng, shape):
    """U[0,1) draws [N, A, H, U] that hold an exact 0 and the largest fp32 below 1 in every action dimension, at particles /
    agents / planning steps that move with u (the two ends of u * (hi - lo) + lo, random_search.py:40-41, pso.py:143-160)"""
    u01 = rng.random(shape).astype(F)
    n, a, h, nu = shape
    for u in range(nu):
        u01[(2 * u) % n, u % a, u % h, u] = F(0)
        u01[(2 * u + 1) % n, (u + 1) % a, (u + 2) % h, u] = ONE_BELOW
    return u01


def make_noise(opt_name, rng, num_agents, U, n=N, h=H, iters=ITERS):
    """the standard draws of ONE control step, in the oracle's layouts"""
    shape = (n, num_agents, h, U)
    if opt_name == "RS":
        return {"uniform": edge_uniform(rng, shape)}
    if opt_name in ("CEM", "CEM-warm", "PI2"):
        return {"trunc": [O.truncated_normal_noise(rng, shape) for _ in range(iters)]}
    if opt_name == "SPSA":
        return {"rademacher": [_rademacher(rng, shape) for _ in range(iters)]}
    if opt_name in ("PSO", "PSO-reset"):
        return {"normal2": rng.standard_normal((iters, 2)).astype(F), "trunc": O.truncated_normal_noise(rng, shape),
                "uniform": edge_uniform(rng, shape)}
    return {"normal": [rng.standard_normal(shape).astype(F) for _ in range(iters)]}          # CMA-ES: [iters][N, A, H, U]


def make_reset_noise(rng, num_agents, U, n=N, h=H):
    return {"uniform_pos": edge_uniform(rng, (n, num_agents, h, U)), "uniform_vel": edge_uniform(rng, (n, num_agents, h, U))}


# ---- the oracle, one optimizer per runner ---------------------------------------------------------------------------
def _record_clips(opt, sink):
    """every _clip_h call of the oracle (pi2.py:70-71, spsa.py:78-81, 105-107, pso.py:76-77, cma_es.py:147-148) leaves its
    UNCLIPPED argument in `sink`: what check_candidates and the coverage counts need, without a change to the oracle"""
    orig = opt._clip_h

    def clip(x):
        sink.append(np.array(x, F))
        return orig(x)
    opt._clip_h = clip


class Runner:
    """One optimizer of oracle_np under the given bounds.  step() runs one control step's _optimize with this step's draws
    and, optionally, the lock-step hooks of the GPU tests; `clips` holds, per control step, the unclipped arguments of
    every clip in call order (PI2 / PSO / CMA-ES: one per iteration; SPSA: plus, minus, updated solution per iteration)."""

    def __init__(self, opt_name, ev, lo, hi, num_agents, n=N, h=H, iters=ITERS, k=K, mix=None):
        from tests import correlated_util as CU
        self.mix, self._cu = mix, CU
        self.name, self.A, self.n_pop, self.H, self.iters, self.k = opt_name, num_agents, n, h, iters, k
        self.lo, self.hi = np.asarray(lo, F).reshape(-1), np.asarray(hi, F).reshape(-1)
        self.U = self.lo.shape[0]
        kw = dict(horizon=h, population=n, num_agents=num_agents)
        mk = {"RS": lambda **q: O.RandomSearch(ev, lo, hi, **q),
              "CEM": lambda **q: (O.CEM(ev, lo, hi, max_iterations=iters, num_elite=k, **q) if mix is None else
                                  CU.CorrelatedCEM(ev, lo, hi, max_iterations=iters, num_elite=k, mix=mix, **q)),
              "PI2": lambda **q: O.PI2(ev, lo, hi, max_iterations=iters, **q),
              "SPSA": lambda **q: O.SPSA(ev, lo, hi, max_iterations=iters, **q),
              "PSO": lambda **q: O.PSO(ev, lo, hi, max_iterations=iters, **q),
              "CMA": lambda **q: O.CMAES(ev, lo, hi, max_iterations=iters, num_elite=k, **q)}[opt_name.split("-")[0]]
        if opt_name == "CMA-pa":                          # one instance of n = H U per agent (BBMPC_CMAES_PER_AGENT)
            kw["num_agents"] = 1
            self.opts = [mk(**kw) for _ in range(num_agents)]
        else:
            self.opts = [mk(**kw)]
        self.opt = self.opts[0]
        self.clips, self._sink = [], []
        for o in self.opts:
            _record_clips(o, self._sink)

    def reset(self, noise):
        assert self.name == "PSO-reset"
        self.opt.reset(noise)

    def step(self, state, noise, **lock):
        """-> action [A, U].  lock: forced_elites (CEM), rewards_override (PI2, PSO), eig / forced_order (CMA-ES; lists
        over the instances in per-agent mode)"""
        state = np.asarray(state, F)
        del self._sink[:]
        if self.name == "CMA-pa":
            acts = []
            for a, o in enumerate(self.opts):
                z = [x[:, a].reshape(self.n_pop, -1) for x in noise["normal"]]
                q = {key: v[a] for key, v in lock.items()}
                acts.append(o._optimize(state[a:a + 1], {"normal": z}, **q))
            act = np.concatenate(acts, 0)
        elif self.name == "CMA":
            act = self.opt._optimize(state, {"normal": [x.reshape(self.n_pop, -1) for x in noise["normal"]]}, **lock)
        else:
            if self.mix is not None and self.name == "PI2":       # PI2 takes the mixed draws as its noise; CorrelatedCEM mixes itself
                noise = self._cu.mixed_noise(self.mix, noise)
            act = self.opt._optimize(state, noise, **lock)
            if self.name == "CEM-warm":                   # BBMPC_FIX_Q2_CEM_WARM_START: the assignment cem.py:133-134 comments out
                self.opt.prev = self.opt.trace[-1]["mean"].copy()
        self.clips.append([c.copy() for c in self._sink])
        return np.array(act, F)

    def prev_mean(self):
        """what the next control step starts from ([A, H, U]), where the optimizer keeps one"""
        if self.name in ("CEM", "CEM-warm", "PI2"):
            return self.opt.prev
        if self.name == "SPSA":
            return self.opt.params
        return None


# ---- coverage: what a run of the oracle exercised --------------------------------------------------------------------
def clip_coverage(clips, lo, hi, atol=1e-5):
    """clips: unclipped candidate tensors [..., (A,) H, U] of any number of clip calls.  Per action dimension: elements
    clipped at hi, at lo, and population rows ([..., A] entries) whose penalty |x - clip(x)|^2 is non-zero because of that
    dimension."""
    lo64, hi64 = _b(lo), _b(hi)
    nu = lo64.shape[0]
    at_hi, at_lo, pen = np.zeros(nu, np.int64), np.zeros(nu, np.int64), np.zeros(nu, np.int64)
    for x in clips:
        x = np.asarray(x, np.float64)
        over, under = x > hi64 + atol, x < lo64 - atol
        at_hi += over.reshape(-1, nu).sum(0)
        at_lo += under.reshape(-1, nu).sum(0)
        pen += (over | under).any(axis=-2).reshape(-1, nu).sum(0)          # any planning step of the row
    return dict(at_hi=at_hi, at_lo=at_lo, penalised=pen)


def constrained_variance(mean, var, lo, hi):
    """min(((mean - lo) / 2)^2, ((hi - mean) / 2)^2, var) of cem.py:79-88 / pso.py:116-120 in fp32, and which arm is the
    smaller bound arm"""
    lo_h, hi_h = np.asarray(lo, F).reshape(-1), np.asarray(hi, F).reshape(-1)
    lb, ub = (mean - lo_h).astype(F), (hi_h - mean).astype(F)
    cv = np.minimum(np.minimum(((lb / F(2)) ** 2).astype(F), ((ub / F(2)) ** 2).astype(F)), var)
    return cv, lb < ub, ub < lb


def variance_coverage(runner):
    """Elements whose constrained variance is STRICTLY below the unconstrained one, split by the nearer bound
    (lo: mean - lo < hi - mean).  CEM: iterations >= 1 of the last control step run, against the refit variance;
    PSO: the post-loop re-seed (pso.py:116-120), against the constant variance."""
    o = runner.opt
    near_lo = near_hi = 0
    if runner.name.startswith("CEM"):
        for it in range(1, runner.iters):
            mean, var = o.trace[it - 1]["mean"], o.trace[it - 1]["var"]
            cv, lo_side, hi_side = constrained_variance(mean, var, runner.lo, runner.hi)
            np.testing.assert_array_equal(cv, o.trace[it]["cvar"])
            near_lo += int(((cv < var) & lo_side).sum())
            near_hi += int(((cv < var) & hi_side).sum())
    else:
        cv, lo_side, hi_side = constrained_variance(o.gbest, o.var, runner.lo, runner.hi)
        near_lo, near_hi = int(((cv < o.var) & lo_side).sum()), int(((cv < o.var) & hi_side).sum())
    return dict(near_lo=near_lo, near_hi=near_hi)


# ---- one case: the draws of its control steps and the free-running oracle over them ------------------------------------
def case_draws(opt_name, num_agents, U, seed, steps=STEPS, n=N, h=H, iters=ITERS):
    """(reset draws or None, [per control step draws]): the same for the CPU and the GPU tests of a case"""
    rng = np.random.default_rng(seed)
    reset = make_reset_noise(rng, num_agents, U, n, h) if opt_name == "PSO-reset" else None
    return reset, [make_noise(opt_name, rng, num_agents, U, n, h, iters) for _ in range(steps)]


def run_oracle(opt_name, ev, lo, hi, states, seed, n=N, h=H, iters=ITERS, k=K, mix=None):
    """the free-running oracle over the case's control steps -> (runner, per-step variance coverage or None)"""
    steps, num_agents = states.shape[0], states.shape[1]
    r = Runner(opt_name, ev, lo, hi, num_agents, n, h, iters, k, mix)
    reset, draws = case_draws(opt_name, num_agents, r.U, seed, steps, n, h, iters)
    if reset is not None:
        r.reset(reset)
    var_cov = []
    for t in range(steps):
        r.step(states[t], draws[t])
        if (opt_name.startswith("CEM") and mix is None) or opt_name.startswith("PSO"):
            var_cov.append(variance_coverage(r))
    return r, var_cov
