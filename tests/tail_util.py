"""The tail of OptimizerBase.__call__ (optimizer_base.py:82-94) restated in float64 NumPy: exploration noise + clip, the
warm-start shift, and the designed bounds / noise sets the tail tests share.  Test infrastructure only.

The reference takes the device's PRE-noise action as given; the model step is not restated here (the oracle's
pendulum / MLP step evaluates the device's own noisy action)."""
import numpy as np

from oracle import oracle_np as O
from tests import philox_np as P

F = np.float32
EXPLORATION_STREAM = 10                      # BBMPC_NOISE_EXPLORATION


def _f64(x):
    return np.asarray(x, np.float64)


def _b(x):
    """bounds as the engine holds them: rounded to fp32 first"""
    return np.asarray(x, F).astype(np.float64).reshape(-1)


def exploration_std(lo, hi):
    lo, hi = _b(lo), _b(hi)
    return np.sqrt((lo - hi) ** 2 / 16.0 * 0.05)                 # optimizer_base.py:46-48


def exploration_unclipped(action, xi, lo, hi, fix_q7):
    lo, hi = _b(lo), _b(hi)
    mean = np.zeros_like(lo) if fix_q7 else (hi + lo) / 2.0      # :49-50 (quirk Q7: the bounds midpoint)
    return _f64(action) + _f64(xi) * exploration_std(lo, hi) + mean


def exploration(action, xi, lo, hi, fix_q7):
    """clip(action + xi * sqrt((lo-hi)^2/16*0.05) + (0 if fix_q7 else (hi+lo)/2), lo, hi), bounds per dimension, float64."""
    lo, hi = _b(lo), _b(hi)
    return np.clip(exploration_unclipped(action, xi, lo, hi, fix_q7), lo, hi)            # :83-90


def exploration_xi(seed, step, A, U, agent_offset=0):
    """The documented production draw [A, U]: stream 10, counter (0, ga*ceil(U/4) + (u>>2), control step, 10<<16), output
    word u & 3, through the truncated-normal table."""
    return P.trunc_normal(P.words(seed, step, EXPLORATION_STREAM, 0, 1, A, U, agent_offset))[0]


def shift_left(mean):
    """pi2.py:92-93 / spsa.py:114-115: [A, H, U] -> the plan moved one step forward, the last step repeated."""
    mean = np.asarray(mean)
    return np.concatenate([mean[:, 1:], mean[:, -1:]], axis=1)


def action_atol(action, xi, lo, hi, fix_q7):
    """Per-element bound on |fp32 exploration_action - float64 reference|.  The device computes d = lo - hi, d*d, /16
    (exact), *0.05f, sqrt, xi*sd, hi+lo, /2 (exact), + mean, act + noise: at most 8 correctly rounded fp32 operations (0.05f
    itself counts as one) on magnitudes no larger than M = max(|lo|, |hi|, |action|) + |noise| + |mid|, so
    atol = 8 * 2^-24 * M and rtol = 0."""
    lo, hi = _b(lo), _b(hi)
    mid = np.zeros_like(lo) if fix_q7 else np.abs(hi + lo) / 2.0
    m = np.maximum(np.maximum(np.abs(lo), np.abs(hi)), np.abs(_f64(action))) + np.abs(_f64(xi)) * exploration_std(lo, hi) + mid
    return 8.0 * 2.0 ** -24 * m


def check_action(got, action, xi, lo, hi, fix_q7, what=""):
    """got (fp32, the noisy engine's action) against the reference: within action_atol, and exactly the bound wherever the
    reference clips by more than that bound on the error.  Returns (clipped at hi, clipped at lo, inside) counts."""
    lo64, hi64 = _b(lo), _b(hi)
    raw = exploration_unclipped(action, xi, lo, hi, fix_q7)
    want = np.clip(raw, lo64, hi64)
    tol = action_atol(action, xi, lo, hi, fix_q7)
    got64 = _f64(got)
    err = np.abs(got64 - want)
    assert got64.shape == want.shape, (what, got64.shape, want.shape)
    assert np.all(err <= tol), "%s: exploration action off by %s (bound %s) at %s\n got  %s\n want %s" % (
        what, err.max(), tol.flat[int(np.argmax(err - tol))], np.unravel_index(int(np.argmax(err - tol)), err.shape), got64, want)
    at_hi, at_lo = raw > hi64 + tol, raw < lo64 - tol
    hi_b, lo_b = np.broadcast_to(hi64, raw.shape), np.broadcast_to(lo64, raw.shape)
    assert np.array_equal(got64[at_hi], hi_b[at_hi]), "%s: clipped elements must equal hi exactly" % what
    assert np.array_equal(got64[at_lo], lo_b[at_lo]), "%s: clipped elements must equal lo exactly" % what
    assert np.all(got64 >= lo_b) and np.all(got64 <= hi_b), "%s: action outside the bounds" % what
    inside = (raw < hi64 - tol) & (raw > lo64 + tol)
    return int(at_hi.sum()), int(at_lo.sum()), int(inside.sum())


# ---- designed inputs ---------------------------------------------------------------------------------------------
# Pendulum (U = 1).  The noise is at most 2 * 0.0559 * (hi - lo) wide, so with draws inside (-2, 2) whether an element clips
# depends on where the optimizer's action lies.  Every designed set therefore carries, besides values near +-2, near 0 and
# random ones, two FORCING elements (xi = +-FORCE, far outside what the sampler can draw): FORCE * sd = 4.47 * (hi - lo), more
# than the range plus the largest |midpoint| used here (1.5 * range), so those elements clip at hi and at lo whatever action
# in [lo, hi] the optimizer returns, under Q7 and under FIX_Q7.
FORCE = 80.0
PENDULUM_BOUNDS = {
    "sym": ([-2.0], [2.0]),          # midpoint 0: Q7 and FIX_Q7 coincide (the one case the older test covers)
    "asym": ([-0.5], [1.5]),         # midpoint 0.5 = 4.5 sd: with draws in (-2, 2) the Q7 noise is always positive -> never clips at lo
    "pos": ([0.5], [1.5]),           # lo > 0, midpoint 1.0 = hi - lo: Q7 alone saturates every in-distribution row at (or next to) hi
}
MLP_BOUNDS = {                       # per-dimension, asymmetric, (lo[u], hi[u]) different for every u
    2: ([-0.5, 0.25], [1.5, 0.75]),
    6: ([-1.0, -0.5, 0.25, -0.75, -0.2, -1.0], [1.0, 1.5, 0.75, 0.25, 0.6, -0.5]),
}


def wide_bounds(U):
    """U > 6: lo[u] and hi[u] distinct for every u, mixed signs of the midpoint, one dimension in four with lo > 0."""
    u = np.arange(U, dtype=np.float64)
    lo = -1.0 + 0.013 * u + np.where(u % 4 == 3, 1.25, 0.0)
    hi = lo + 0.5 + 0.017 * u
    return lo.astype(F), hi.astype(F)


def designed_xi(A, U, seed):
    """[A, U] fp32: one element near +2, one near -2, one near 0, the forcing pair, the rest uniform in (-2, 2).  The five
    designed values sit at flattened (a, u) indices (5 i + seed) mod A U, so they move to other agents and dimensions from one
    control step to the next; where 5 divides A U (or A U <= 5) they take the first indices instead.  With fewer than five
    elements (the pendulum at A = 1 and A = 3) only the first A U of them fit and the forcing pair is left out: the tests
    assert clip coverage at the sizes of tests/test_tail_cpu.py only."""
    rng = np.random.default_rng(seed)
    xi = rng.uniform(-1.999, 1.999, A * U)
    special = [1.9995, -1.9995, 1e-3, FORCE, -FORCE]
    n = A * U
    for i, v in enumerate(special):
        if i < n:
            xi[(i * 5 + seed) % n if n > 5 and np.gcd(5, n) == 1 else i] = v
    return xi.reshape(A, U).astype(F)


# ---- the problems the tail tests and the bounds tests share: states, user functions, learned models --------------
def pendulum_states(steps, A, seed):
    rng = np.random.default_rng(seed)
    th = rng.uniform(-np.pi, np.pi, (steps, A))
    return np.stack([np.cos(th), np.sin(th), rng.uniform(-6, 6, (steps, A))], -1).astype(F)


INTENDED_PENDULUM_REWARD = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    const float PI = 3.14159274101257324f, TWO_PI = 6.28318548202514648f;
    const float th = atan2f(cur[1], cur[0]);
    float m = fmodf(th + PI, TWO_PI);
    if (m < 0.0f) m = m + TWO_PI;
    const float ang = m - PI;
    const float first = ang * ang + 0.1f * (cur[2] * cur[2]);
    float ss = 0.0f;
    for (int u = 0; u < U; ++u) ss = ss + act[u] * act[u];
    return (-first) - 0.001f * ss;
}
"""
# a linear model with two inputs: delta[i] = 0.05 * act[i % U] - 0.01 * x[i]
LINEAR_DYNAMICS = """
__device__ void bbmpc_user_dynamics(const float* x, float* delta, int S, int U) {
    for (int i = 0; i < S; ++i) delta[i] = 0.05f * x[S + (i % U)] - 0.01f * x[i];
}
"""


def linear_dynamics_np(x):
    x = np.asarray(x, F)
    S, U = 3, x.shape[1] - 3
    return np.stack([(F(0.05) * x[:, S + (i % U)]).astype(F) - (F(0.01) * x[:, i]).astype(F) for i in range(S)], 1).astype(F)


def intended_reward(cur, act, nxt):
    return O.pendulum_reward(cur, act, nxt, as_executed=False)


ACT = {"tanh": 1, "relu": 2, "sigmoid": 3, None: 0}
MLP_SHAPES = {
    "S20-U6-h200": ([26, 200, 200, 20], ["tanh", "tanh", None], 20, 6, "cheetah"),
    "S3-U2-h16": ([5, 16, 3], ["tanh", None], 3, 2, "pendulum"),
    # the two corners of what bbmpc_set_mlp accepts (dim_S + dim_U <= 128 and dim_S <= 64).  Widest state: k_tail_mlp's state
    # threads 64..64+S are all in use.  Widest action: its action threads 64..64+U and tid < U run far past the state range, act[128]
    # is all but full, and a production draw takes 32 Philox blocks per agent
    "S64-U64-h96": ([128, 96, 64], ["tanh", None], 64, 64, "cheetah"),
    "S3-U125-h96": ([128, 96, 3], ["tanh", None], 3, 125, "pendulum"),
}


def mlp_stats(S, U, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 0.2, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F),
            rng.normal(0, 0.1, U).astype(F), rng.uniform(0.5, 1.5, U).astype(F),
            rng.normal(0, 0.01, S).astype(F), rng.uniform(0.05, 0.15, S).astype(F)]


_NETS = {}


def net(shape, normalized):
    """weights / statistics / oracle evaluator of a shape: made once, shared by the cases, never changed"""
    key = (shape, normalized)
    if key not in _NETS:
        dims, acts, S, U, reward = MLP_SHAPES[shape]
        ws, bs = O.make_mlp_params(dims, seed=42)
        rng = np.random.default_rng(43)
        bs = [rng.normal(0, 0.05, b.shape).astype(F) for b in bs]
        stats = mlp_stats(S, U, 44) if normalized else None
        ev = O.Evaluator(reward, O.Handler(O.MLP(ws, bs, acts), False, normalized, stats))
        _NETS[key] = (ws, bs, stats, ev)
    return _NETS[key]


def mlp_bounds(U):
    lo, hi = MLP_BOUNDS[U] if U in MLP_BOUNDS else wide_bounds(U)
    return np.asarray(lo, F), np.asarray(hi, F)


def mlp_states(shape, steps, A, seed):
    S = MLP_SHAPES[shape][2]
    if S == 3:
        return pendulum_states(steps, A, seed)
    return np.random.default_rng(seed).normal(0, 0.3, (steps, A, S)).astype(F)
