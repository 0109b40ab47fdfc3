"""NumPy statements of the particle evaluator's CVaR score and nearest-rank quantiles (include/bbmpc.h:
bbmpc_set_particle_risk, bbmpc_predict_trajectory_quantiles) for the tests.  The stable rank is written as its definition

    rank[p] = #{q : x[q] < x[p]} + #{q < p : x[q] == x[p]}

-- an O(P^2) count, not a sort -- and everything else is selection by that rank."""
import numpy as np

from oracle import oracle_np as O

F = np.float32


def stable_rank(x, axis):
    """Ranks 0 .. P-1 along `axis`, equal values ordered by index; same shape as x (int64)."""
    x = np.moveaxis(np.asarray(x), axis, -1)
    p = x.shape[-1]
    xp, xq = x[..., :, None], x[..., None, :]                  # [.., p, q]
    earlier = np.arange(p)[None, :] < np.arange(p)[:, None]    # [p, q]: q < p
    rank = (xq < xp).sum(axis=-1) + ((xq == xp) & earlier).sum(axis=-1)
    return np.moveaxis(rank, -1, axis)


def cvar32(returns, k):
    """[N, P, A] -> [N, A]: the fp32 sum of the k lowest-ranked returns, added in particle index order, over float32(k)."""
    r = O.f32(returns)
    sel = stable_rank(r, 1) < k
    total = np.zeros((r.shape[0], r.shape[2]), F)
    for p in range(r.shape[1]):                                # index order; particles outside the tail add nothing at all
        total = np.where(sel[:, p], (total + r[:, p]).astype(F), total)
    return (total / F(k)).astype(F)


def cvar64(returns, k):
    r = np.asarray(returns, np.float64)
    return np.sort(r, axis=1)[:, :k].mean(axis=1)


def nearest_rank(x, ranks, axis):
    """The values of x whose stable rank along `axis` is ranks[l]: `axis` is replaced by the levels."""
    x = np.moveaxis(np.asarray(x), axis, -1)
    rank = stable_rank(x, -1)
    out = np.stack([np.where(rank == r, x, 0).sum(axis=-1, dtype=x.dtype) for r in ranks], axis=-1)    # one match per row
    return np.moveaxis(out, -1, axis)
