"""NumPy statements for the trajectory-distribution tests (include/bbmpc.h: bbmpc_predict_trajectory_particles), on
tests/particle_util.py, gaussian_util.py and traj_util.py: the particle recurrence from every row's own start state,

    s_0 = states[b];  nxt = predict_next_state_member(p % E)(s_t, a[b,t]) + (sigma + sd(s_t, a[b,t])) * eps[b,p,t,:]
    particle_states[b,p,t] = nxt;  particle_rewards[b,p,t] = reward(s_t, a[b,t], nxt);  s_{t+1} = nxt

in float32 (one rounding per op) with the oracle's evaluators, in lock step with a device's own states, and the per-step
moments over the particles in float32 (index order, as k_particle_aggregate) and float64."""
import numpy as np

from oracle import oracle_np as O
from tests import traj_util as T

F = np.float32
LOCK_RTOL, LOCK_ATOL = 2e-5, 2e-5          # the one-step state tolerance of tests/test_gpu_mlp.py (traj_util.STATE_*)


def oracle_step(ev, head, s, a, sigma, e):
    """One noisy step in float32: ev.predict_next_state + (sigma [+ head.sd32]) * e."""
    nxt = ev.predict_next_state(s, a)
    scale = O.f32(sigma) if head is None else (O.f32(sigma) + head.sd32(s, a)).astype(F)
    return (nxt + (scale * O.f32(e)).astype(F)).astype(F)


def oracle_particles(evs, heads, states, seq, eps, sigma):
    """The recurrence with member p % E: (particle_states [B,P,Hq,S], particle_rewards [B,P,Hq]) float32."""
    states, seq, eps = O.f32(states), O.f32(seq), O.f32(eps)
    B, P, Hq, S = eps.shape
    E = len(evs)
    ps, pr = np.empty((B, P, Hq, S), F), np.empty((B, P, Hq), F)
    for p in range(P):
        ev, head = evs[p % E], (heads[p % E] if heads else None)
        s = states
        for t in range(Hq):
            nxt = oracle_step(ev, head, s, seq[:, t], sigma, eps[:, p, t])
            pr[:, p, t] = ev.evaluate_next_reward(s, nxt, seq[:, t])
            ps[:, p, t] = nxt
            s = nxt
    return ps, pr


def check_lockstep(evs, heads, states, seq, eps, sigma, got_ps, got_pr, what):
    """Every returned state against the oracle's step FROM THE DEVICE'S OWN previous state (rtol / atol of one step), every
    reward against the oracle's reward on the device's own states (rtol 1e-4, atol 1e-3: an indicator cannot fall
    differently).  Prints the largest deviations first."""
    states, seq, eps = O.f32(states), O.f32(seq), O.f32(eps)
    B, P, Hq, S = eps.shape
    E = len(evs)
    assert got_ps.shape == (B, P, Hq, S) and got_pr.shape == (B, P, Hq)
    ds = dr = 0.0
    want_s, want_r = np.empty_like(got_ps), np.empty_like(got_pr)
    for p in range(P):
        ev, head = evs[p % E], (heads[p % E] if heads else None)
        for t in range(Hq):
            cur = states if t == 0 else got_ps[:, p, t - 1]
            want_s[:, p, t] = oracle_step(ev, head, cur, seq[:, t], sigma, eps[:, p, t])
            want_r[:, p, t] = ev.evaluate_next_reward(cur, got_ps[:, p, t], seq[:, t])
    ds = np.abs(got_ps.astype(np.float64) - want_s).max()
    dr = np.abs(got_pr.astype(np.float64) - want_r).max()
    print("[%s] lock step: max |state dev| %.3e, max |reward dev| %.3e" % (what, ds, dr))
    np.testing.assert_allclose(got_ps, want_s, rtol=LOCK_RTOL, atol=LOCK_ATOL)
    np.testing.assert_allclose(got_pr, want_r, rtol=T.REWARD_RTOL, atol=T.REWARD_ATOL)


def particles64(step64, states, seq, eps, sigma):
    """One model in float64 with the pendulum reward (as executed): step64(s, u) -> next, traj_util's forms."""
    states, seq, eps = (np.asarray(v, np.float64) for v in (states, seq, eps))
    B, P, Hq, S = eps.shape
    sigma = np.asarray(sigma, np.float64)
    ps, pr = np.empty((B, P, Hq, S)), np.empty((B, P, Hq))
    for p in range(P):
        s = states
        for t in range(Hq):
            nxt = step64(s, seq[:, t]) + sigma * eps[:, p, t]
            pr[:, p, t] = T.pendulum_reward64(s, nxt, seq[:, t], True)
            ps[:, p, t] = nxt
            s = nxt
    return ps, pr


def steps_first(x):
    """[B,P,Hq,...] -> [B*P,Hq,...]: the layout traj_util.check_against_float64 takes its per-step maxima over."""
    return x.reshape((x.shape[0] * x.shape[1],) + x.shape[2:])


# ---- moments over the particle axis (axis 1) ----------------------------------------------------------------------------
def moments32(x):
    """(mean, std) in float32, sums over p in index order: mean = (sum x) / P, std = sqrt(sum (x - mean)^2 / P)."""
    x = O.f32(x)
    P = x.shape[1]
    mean = (O.seq_sum(x, axis=1) / F(P)).astype(F)
    d = (x - mean[:, None]).astype(F)
    var = (O.seq_sum((d * d).astype(F), axis=1) / F(P)).astype(F)
    return mean, O.sqrt32(var)


def moments64(x):
    x = np.asarray(x, np.float64)
    return x.mean(axis=1), x.std(axis=1)


def moments_bound(x):
    """particle_util.aggregate_bound at kappa = 1 per output element: 64 P 2^-24 * 2 * max_p |x_p|, and for the std the
    elements where it may be asserted (the float64 std is at least 1 % of max_p |x_p|: d sqrt(v) ~ dv / (2 sqrt(v)))."""
    x = np.asarray(x, np.float64)
    big = np.abs(x).max(axis=1)
    return 64.0 * x.shape[1] * 2.0 ** -24 * 2.0 * big, x.std(axis=1) >= 0.01 * big


def check_moments(got_mean, got_std, x, what):
    """Device moments against the float32 restatement of the device's own particle tensor `x`, at aggregate_bound's size;
    the std where the bound is meaningful, and never negative or NaN."""
    m32, s32 = moments32(x)
    bound, rows = moments_bound(x)
    em = np.abs(got_mean.astype(np.float64) - m32)
    es = np.abs(got_std.astype(np.float64) - s32)
    print("[%s] moments: max |mean - restatement| %.3e, max |std - restatement| %.3e (bound >= %.3e), identical bits: %s / %s"
          % (what, em.max(), es.max(), bound.min(), np.array_equal(got_mean, m32), np.array_equal(got_std, s32)))
    assert np.all(em <= bound)
    assert np.all(es[rows] <= bound[rows])
    assert np.all(got_std >= 0)


# ---- cases ----------------------------------------------------------------------------------------------------------------
def rows_for(c, B, Hq, seed):
    """B start states and sequences of Hq steps for the network of traj_util case `c` (its recipe, any B and Hq)."""
    rng = np.random.default_rng(seed)
    states = (rng.standard_normal((B, c["S"])) * 0.3).astype(F)
    states[:, 0] += F(1.0)
    return states, rng.uniform(-1, 1, (B, Hq, c["U"])).astype(F)
