"""StateBoxTermination -- an episode ends when the state leaves a box.

The termination predicate of the shaped returns (bbmpc_set_return_shaping): a candidate's rollout
stops at the first model state with any coordinate below `low` or above `high`, collects `terminal_reward` there and
takes no terminal value.  gym's "healthy range" conditions (Hopper, Walker, a speed limit) are boxes of this kind.
`__call__` states the same predicate on NumPy arrays; a NaN coordinate is never outside (both comparisons are false)."""
import numpy as np


class StateBoxTermination:
    def __init__(self, low=None, high=None, terminal_reward=0.0):
        """low / high: arrays of length dim_S or scalars; None or -inf / +inf means unbounded."""
        self._version = 0
        self._low = self._high = None
        self._terminal_reward = 0.0
        self.set_bounds(low, high)
        self.terminal_reward = terminal_reward

    @staticmethod
    def _bound(v, unbounded):
        if v is None:
            return np.float32(unbounded)
        b = np.asarray(v, np.float32)
        if b.ndim > 1:
            raise ValueError("a bound is a scalar or a [dim_S] vector, got shape %s" % (b.shape,))
        if np.any(np.isnan(b)):
            raise ValueError("a bound must not be NaN (None or -inf / +inf mean unbounded)")
        return b.copy()

    def set_bounds(self, low=None, high=None):
        """Replace both bounds; every engine that holds the box uploads it again before its next computation."""
        lo, hi = self._bound(low, -np.inf), self._bound(high, np.inf)
        if lo.ndim == 1 and hi.ndim == 1 and lo.shape != hi.shape:
            raise ValueError("low %s and high %s differ in length" % (lo.shape, hi.shape))
        if np.any(lo > hi):
            raise ValueError("low must not exceed high")
        self._low, self._high = lo, hi
        self._version += 1

    @property
    def low(self):
        return self._low

    @property
    def high(self):
        return self._high

    @property
    def terminal_reward(self):
        return self._terminal_reward

    @terminal_reward.setter
    def terminal_reward(self, value):
        c = float(value)
        if not np.isfinite(c):
            raise ValueError("terminal_reward must be finite, got %r" % (value,))
        self._terminal_reward = c
        self._version += 1

    def bounds(self, dim_S):
        """(low [dim_S], high [dim_S]) float32, scalars broadcast."""
        out = []
        for b in (self._low, self._high):
            if b.ndim == 1 and b.shape != (int(dim_S),):
                raise ValueError("the box has %d coordinates but the state has %d" % (b.shape[0], int(dim_S)))
            out.append(np.ascontiguousarray(np.broadcast_to(b, (int(dim_S),)), np.float32))
        return out[0], out[1]

    def __call__(self, states):
        """states [..., dim_S] -> bool [...]: any coordinate below low or above high."""
        s = np.asarray(states)
        lo, hi = self.bounds(s.shape[-1])
        with np.errstate(invalid="ignore"):
            return np.any((s < lo) | (s > hi), axis=-1)
