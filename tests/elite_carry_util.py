"""NumPy statement of CEM's elite carry-over (include/bbmpc.h bbmpc_set_elite_carry), shared by
tests/test_elite_carry_cpu.py and tests/test_gpu_elite_carry.py.

With E_i[a] the sorted elite list of iteration i and X_i[n,a,t,u] the candidates of iteration i as rolled out:
    keep:   X_i[N - keep + e, a]        = X_{i-1}[E_{i-1}[a][e], a]                      for i >= 1 within a control step
    shift:  X_0[N - shift + e, a, t, :] = X_L[E_L[a][e], a, min(t + 1, H - 1), :]        L = the previous step's last iteration
after the draw of that iteration; everything else is the optimizer it is built on.
"""
import numpy as np

from oracle import oracle_np as O
from tests import correlated_util as CU

F = np.float32


def gather_elites(samples, idx, count):
    """samples [N,A,H,U], idx [A,k] -> the first `count` elite rows of every agent, [count,A,H,U] (copies)."""
    A = samples.shape[1]
    return np.stack([samples[idx[a][:count], a] for a in range(A)], axis=1).copy()


def shift_rows(rows):
    """[..., H, U] moved one planning step forward, the last step repeated."""
    return np.concatenate([rows[..., 1:, :], rows[..., -1:, :]], axis=-2)


class _CarryMixin:
    """_optimize with the two overwrites; the class it is mixed into supplies `_candidates` (its own draw)."""

    def _init_carry(self, keep, shift):
        assert 0 <= keep <= self.k and 0 <= shift <= self.k and max(keep, shift) < self.N
        self.keep, self.shift = int(keep), int(shift)
        self.stored = None                                  # [shift,A,H,U] for the next control step, or None

    def reset(self):
        super().reset()
        self.stored = None

    def _optimize(self, state, noise, forced_elites=None):
        mean, var = self.prev.copy(), self.var0.copy()
        self.trace = []
        carried, self.stored = self.stored, None
        for it in range(self.iters):
            samples = self._candidates(mean, var, noise["trunc"][it])
            if carried is not None and len(carried):
                samples[self.N - len(carried):] = carried                      # the last columns, bit for bit
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
            if it + 1 < self.iters:
                carried = gather_elites(samples, idx, self.keep)
            elif self.shift:
                self.stored = shift_rows(gather_elites(samples, idx, self.shift))
        return mean[:, 0]


class _PlainCarryCEM(_CarryMixin, O.CEM):
    def _candidates(self, mean, var, z):                    # oracle_np.CEM's draw (cem.py:79-94)
        sigma = CU.cem_sigma32(mean, var, self.lo_h, self.hi_h)
        return ((O.f32(z) * sigma).astype(F) + mean).astype(F)


class _CorrelatedCarryCEM(_CarryMixin, CU.CorrelatedCEM):
    def _candidates(self, mean, var, z):                    # correlated_util.CorrelatedCEM's draw: mixed, then clipped
        sigma = CU.cem_sigma32(mean, var, self.lo_h, self.hi_h)
        return self._clip_h(((CU.mix32(self.mix, z) * sigma).astype(F) + mean).astype(F))


def CarryCEM(*args, keep=0, shift=0, mix=None, **kw):
    """oracle_np.CEM (mix = None) or correlated_util.CorrelatedCEM with the elite carry-over: same arguments, the same
    `forced_elites` hook; the stored elites stay on the object across _optimize calls and reset() drops them."""
    cem = _PlainCarryCEM(*args, **kw) if mix is None else _CorrelatedCarryCEM(*args, mix=mix, **kw)
    cem._init_carry(keep, shift)
    return cem
