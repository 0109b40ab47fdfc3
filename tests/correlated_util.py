"""NumPy statements of temporally correlated sampling (include/bbmpc.h bbmpc_set_sampling_correlation),
shared by tests/test_correlated_cpu.py and tests/test_gpu_correlated.py.

    y[n,a,t,u] = sum over s = 0..H-1, ascending, of M[t,s] * z[n,a,s,u]
    x[n,a,t,u] = y * sigma[a,t,u] + mean[a,t,u]          CEM: x clipped to the bounds; PI2: unchanged from there on
"""
import numpy as np

from oracle import oracle_np as O

F = np.float32


def mix32(M, z):
    """The rule in float32, one rounding per product and per sum: M [H,H], z [N,A,H,U] -> y [N,A,H,U]."""
    M, z = np.asarray(M, F), np.asarray(z, F)
    H = M.shape[0]
    assert M.shape == (H, H) and z.shape[2] == H
    y = np.empty_like(z)
    for t in range(H):
        acc = (M[t, 0] * z[:, :, 0, :]).astype(F)
        for s in range(1, H):
            acc = (acc + (M[t, s] * z[:, :, s, :]).astype(F)).astype(F)
        y[:, :, t, :] = acc
    return y


def mix64(M, z):
    """The same sum in float64 (exact products of float32 inputs, 53-bit sums)."""
    M, z = np.asarray(M, np.float64), np.asarray(z, np.float64)
    H = M.shape[0]
    y = np.zeros_like(z)
    for t in range(H):
        for s in range(H):
            y[:, :, t, :] += M[t, s] * z[:, :, s, :]
    return y


def mix_abs64(M, z):
    """sum_s |M[t,s] * z[s]| in float64: the magnitude the sequential-sum error bound is stated in."""
    return mix64(np.abs(np.asarray(M, np.float64)), np.abs(np.asarray(z, np.float64)))


def cem_sigma32(mean, var, lo_h, hi_h):
    """CEM's constrained standard deviation (cem.py:79-88), float32 as oracle_np.CEM computes it."""
    lb = (mean - lo_h).astype(F)
    ub = (hi_h - mean).astype(F)
    cv = np.minimum(np.minimum(((lb / F(2)) ** 2).astype(F), ((ub / F(2)) ** 2).astype(F)), var)
    return O.sqrt32(cv)


def candidates64(M, z, sigma, mean, lo=None, hi=None):
    """(x, magnitude) of the rule in float64 from float32 inputs: x [N,A,H,U] (clipped when lo / hi are given),
    magnitude = sigma * sum_s |M[t,s] z[s]|."""
    y = mix64(M, z)
    x = y * np.asarray(sigma, np.float64)[None] + np.asarray(mean, np.float64)[None]
    raw = x
    if lo is not None:
        x = np.clip(x, np.asarray(lo, np.float64), np.asarray(hi, np.float64))
    return x, mix_abs64(M, z) * np.asarray(sigma, np.float64)[None], raw


def sample_bound(H, magnitude, want):
    """|got - want| <= 2^-23 * ((H + 2) * sigma * sum_s |M[t,s] z[s]| + |want|): the sequential-sum error bound (H products
    and H - 1 sums of relative error 2^-24 each, then one product and one sum of the affine step) with a factor 2 of slack;
    it holds with or without FMA contraction."""
    return 2.0 ** -23 * ((H + 2) * magnitude + np.abs(want))


class CorrelatedCEM(O.CEM):
    """oracle_np.CEM with the mixed draws and the clip line: noise['trunc'] holds the UNMIXED z, `mix` is M."""

    def __init__(self, *args, mix=None, **kw):
        super().__init__(*args, **kw)
        self.mix = np.asarray(mix, F)

    def _optimize(self, state, noise, forced_elites=None):
        mean, var = self.prev.copy(), self.var0.copy()
        self.trace = []
        for it in range(self.iters):
            sigma = cem_sigma32(mean, var, self.lo_h, self.hi_h)
            xi = mix32(self.mix, noise["trunc"][it])
            samples = ((xi * sigma).astype(F) + mean).astype(F)
            samples = self._clip_h(samples)                                    # the added line: a mixed draw leaves 2 sigma
            rewards = self.ev(state, samples)
            idx = O.topk_desc(rewards.T, self.k)
            if callable(forced_elites):
                idx = np.asarray(forced_elites(it, rewards, idx))
            elif forced_elites is not None:
                idx = np.asarray(forced_elites[it])
            st = samples.transpose(1, 0, 2, 3)
            elites = np.stack([st[a][idx[a]] for a in range(self.A)], 0)
            new_mean = (O.seq_sum(elites, axis=1) / F(self.k)).astype(F)
            dev = (elites - new_mean[:, None]).astype(F)
            new_var = (O.seq_sum((dev * dev).astype(F), axis=1) / F(self.k)).astype(F)
            one_m = (F(1) - self.alpha).astype(F)
            mean = ((self.alpha * mean).astype(F) + (one_m * new_mean).astype(F)).astype(F)
            var = ((self.alpha * var).astype(F) + (one_m * new_var).astype(F)).astype(F)
            self.trace.append(dict(samples=samples, rewards=rewards, elites=idx, mean=mean.copy(), var=var.copy()))
        return mean[:, 0]


def mixed_noise(M, noise):
    """What oracle_np.PI2 takes as its 'trunc' noise: the arithmetic behind it is the unmixed optimizer's."""
    return {"trunc": [mix32(M, z) for z in noise["trunc"]]}
