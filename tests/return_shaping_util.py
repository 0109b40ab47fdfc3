"""Discounted, termination-aware returns (bbmpc_set_return_shaping): the float64 NumPy statement that
tests/test_return_shaping_cpu.py and tests/test_gpu_return_shaping.py share.  Test infrastructure only.

The statement, per candidate: states s_1 .. s_H after every step, step rewards r_0 .. r_{H-1},
discount gamma in (0, 1], bounds lo [S] / hi [S] (-inf / +inf: unbounded), a finite terminal reward c:
    outside(s) = any i: s[i] < lo[i] or s[i] > hi[i]          (false on NaN: a NaN state does not terminate)
    g = 1; alive = true; R = 0; T = 0
    for t = 0 .. H-1:
        R += g * r_t
        if outside(s_{t+1}):  R += g * c;  alive = false;  T = t + 1;  stop
        g *= gamma
    if isnan(R): R = -1e6
    R += base                                                  (-(bound penalty) of the rollout, 0 without one)
    if alive and a value network is installed:  R = R + g * w * V(s_H);  a NaN term -> R = -1e6
Nothing behind the terminal step is read: the loop stops, it does not multiply by zero."""
import numpy as np


def outside(states, lo, hi):
    s = np.asarray(states, np.float64)
    with np.errstate(invalid="ignore"):
        return np.any((s < np.asarray(lo, np.float64)) | (s > np.asarray(hi, np.float64)), axis=-1)


def shaped_return(step_rewards, states, gamma=1.0, lo=None, hi=None, c=0.0, base=None, vterm=None, w=1.0):
    """step_rewards [..., H], states [..., H, S] (the state AFTER every step), base [...] or None, vterm [...] (V of
    states[..., -1, :]) or None -> (R [...] float64, T [...] int32).  Written as the loop of the statement, one candidate
    at a time."""
    r = np.asarray(step_rewards, np.float64)
    s = np.asarray(states, np.float64)
    lead, H, S = r.shape[:-1], r.shape[-1], s.shape[-1]
    lo = np.full(S, -np.inf) if lo is None else np.broadcast_to(np.asarray(lo, np.float64), (S,))
    hi = np.full(S, np.inf) if hi is None else np.broadcast_to(np.asarray(hi, np.float64), (S,))
    r2, s2 = r.reshape(-1, H), s.reshape(-1, H, S)
    b2 = np.zeros(r2.shape[0]) if base is None else np.asarray(base, np.float64).reshape(-1)
    v2 = None if vterm is None else np.asarray(vterm, np.float64).reshape(-1)
    R, T = np.zeros(r2.shape[0], np.float64), np.zeros(r2.shape[0], np.int32)
    for i in range(r2.shape[0]):
        g, alive, tot = np.float64(1.0), True, np.float64(0.0)
        for t in range(H):
            tot = tot + g * r2[i, t]
            if outside(s2[i, t], lo, hi):
                tot = tot + g * np.float64(c)
                alive, T[i] = False, t + 1
                break
            g = g * np.float64(gamma)
        if np.isnan(tot):
            tot = np.float64(-1.0e6)
        tot = tot + b2[i]
        if alive and v2 is not None:
            term = g * np.float64(w) * v2[i]
            tot = np.float64(-1.0e6) if np.isnan(term) else tot + term
        R[i] = tot
    return R.reshape(lead), T.reshape(lead)


def near_bound(states, lo, hi, rel=1e-3):
    """states [..., H, S] -> bool [...]: a candidate any of whose (t, i) lies within rel * max(1, |bound|) of an active
    (finite) bound.  The bound test is a discontinuity: such a candidate may fall on either side in float32."""
    s = np.asarray(states, np.float64)
    S = s.shape[-1]
    near = np.zeros(s.shape[:-2], bool)
    for b in (lo, hi):
        if b is None:
            continue
        b = np.broadcast_to(np.asarray(b, np.float64), (S,))
        act = np.isfinite(b)
        if act.any():
            with np.errstate(invalid="ignore"):
                d = np.abs(s[..., act] - b[act]) <= rel * np.maximum(1.0, np.abs(b[act]))
            near |= d.any(axis=(-1, -2))
    return near
