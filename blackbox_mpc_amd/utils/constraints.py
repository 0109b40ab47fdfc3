"""StateBoxConstraint -- keep the probability that a plan leaves a box of states below a limit.

The chance constraint of the particle evaluator (bbmpc_set_chance_constraint): a candidate is rolled
out once per particle, v is the share of its particles whose noisy state ever has a coordinate below `low` or above `high`,
and the candidate's score loses weight * max(0, v - max_violation).  Unlike utils.termination.StateBoxTermination the box
ends nothing: the rollouts and their returns are what they are without it.  `__call__` states the predicate on NumPy
arrays; a NaN coordinate is never outside (both comparisons are false)."""
import numpy as np


class StateBoxConstraint:
    def __init__(self, low=None, high=None, max_violation=0.0, weight=1e3):
        """low / high: arrays of length dim_S or scalars; None or -inf / +inf means unbounded.  max_violation in [0, 1):
        the share of particles that may leave the box for free.  weight >= 0: the penalty per unit of excess share."""
        self._version = 0
        self._low = self._high = None
        self._max_violation, self._weight = 0.0, 0.0
        self.set_bounds(low, high)
        self.max_violation = max_violation
        self.weight = weight

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
    def max_violation(self):
        return self._max_violation

    @max_violation.setter
    def max_violation(self, value):
        d = float(value)
        if not (np.isfinite(d) and 0.0 <= d < 1.0):
            raise ValueError("max_violation must lie in [0, 1), got %r" % (value,))
        self._max_violation = d
        self._version += 1

    @property
    def weight(self):
        return self._weight

    @weight.setter
    def weight(self, value):
        w = float(value)
        if not (np.isfinite(w) and w >= 0.0):
            raise ValueError("weight must be finite and >= 0, got %r" % (value,))
        self._weight = w
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
