"""The chance constraint of the particle evaluator (include/bbmpc.h: bbmpc_set_chance_constraint), stated for the tests.

Per agent a, candidate n, particle p, with s_1 .. s_H the noisy next states of the particle recurrence (s_0 is not tested):

    out(s)        = any i: s[i] < lo[i] or s[i] > hi[i]         (float64 comparisons; false on NaN)
    first[n,p,a]  = the smallest t in 1 .. H with out(s_t), else 0
    count[n,a]    = #{p : first[n,p,a] != 0}
    v[n,a]        = float32(count) / float32(P)
    score'[n,a]   = score[n,a] - lambda * max(0, v[n,a] - delta)     (float32, one rounding per operation, in this order)

The trajectories come from the NumPy statements of the recurrence (tests/particle_util.py, ensemble_util.py,
gaussian_util.py with keep_states=True); `trajectories` / `member_trajectories` bring their row order to [H, N, P, A, S]."""
import numpy as np

F = np.float32


def outside(states, lo, hi):
    """states [..., S] -> bool [...]: any coordinate below lo or above hi; a NaN coordinate is never outside."""
    s = np.asarray(states, np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore"):
        return np.any((s < lo) | (s > hi), axis=-1)


def first_steps(traj, lo, hi):
    """traj [H, ..., S] (s_1 .. s_H) -> int32 [...]: the smallest t in 1 .. H with out(s_t), else 0."""
    out = outside(traj, lo, hi)                          # [H, ...]
    H = out.shape[0]
    first = np.zeros(out.shape[1:], np.int32)
    for t in range(H, 0, -1):                            # the smallest t is written last
        first = np.where(out[t - 1], np.int32(t), first)
    return first


def violation(first):
    """first [N, P, A] -> v [N, A] float32: float32(count) / float32(P)."""
    first = np.asarray(first)
    count = (first != 0).sum(axis=1)
    return (count.astype(F) / F(first.shape[1])).astype(F)


def penalised(score, v, delta, lam):
    """score' = score - lambda * max(0, v - delta), every operation rounded to float32."""
    excess = np.maximum(F(0.0), (np.asarray(v, F) - F(delta)).astype(F)).astype(F)
    return (np.asarray(score, F) - (F(lam) * excess).astype(F)).astype(F)


def trajectories(visited, N, P, A):
    """particle_util.particle_returns(..., keep_states=True)'s visited states [H+1][B, S], rows b = (n * P + p) * A + a
    -> float64 [H, N, P, A, S] (s_1 .. s_H)."""
    return np.stack([np.asarray(v, np.float64).reshape(N, P, A, -1) for v in visited[1:]])


def member_trajectories(visited_per_member, N, P, A):
    """ensemble_util / gaussian_util's per-member lists (member e rolls the particles e, e + E, ..) -> [H, N, P, A, S]."""
    E = len(visited_per_member)
    parts = [trajectories(v, N, P // E, A) for v in visited_per_member]
    out = np.empty((parts[0].shape[0], N, P, A, parts[0].shape[-1]))
    for e, part in enumerate(parts):
        out[:, :, e::E] = part
    return out


def pick_upper_bound(traj, feature, quantile):
    """An upper bound on one feature, chosen from the trajectories alone: the rows' extremes max_t s_t[feature] are sorted
    and the bound goes into the middle of the widest gap among the five next to the wanted quantile.
    -> (bound, half_gap): no row's extreme lies within half_gap of the bound, so a row violates in every computation whose
    states are within half_gap of these."""
    ext = np.sort(np.nanmax(traj[..., feature], axis=0).reshape(-1))
    k = int(np.clip(round(quantile * (ext.size - 1)), 2, ext.size - 4))
    gaps = ext[k - 1:k + 4] - ext[k - 2:k + 3]
    j = int(np.argmax(gaps)) + k - 2
    return 0.5 * (ext[j] + ext[j + 1]), 0.5 * (ext[j + 1] - ext[j])
