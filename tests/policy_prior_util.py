"""Learned policy prior (bbmpc_set_policy_prior_mlp): the float64 NumPy statement, the test networks,
the restatement of noise stream 12 and the optimizer `PriorCEM` that tests/test_policy_prior_cpu.py (statement alone) and
tests/test_gpu_policy_prior.py (device against statement) share.  Test infrastructure only.

The statement, for a policy with Dense layers (W_l [in, out], b_l, act_l) from S inputs to U outputs and statistics
(mean_in, std_in, mean_out, std_out) or none, K = count, sigma_pi = noise_std:
    pi(s) = y * std_out + mean_out,  y = stack((s - mean_in) / (std_in + float32(1e-7)))        (y itself without statistics)
    for iteration i of control step c, agent a, policy rollout e = 0 .. K-1:
      s_0 = state[a]
      for t = 0 .. H-1:   a_t = clip(pi(s_t) + sigma_pi * xi[i, a, e, t, :], lo, hi)
                          s_{t+1} = the learned model's noise-free step (s_t, a_t)
      X_i[N - c_i - K + e, a, t, :] = a_t
with c_i the carried elites injected in iteration i (tests/elite_carry_util.py; 0 without carry).  xi is stream 12:
counter (e, ga * Qk + (j >> 2), control_step, (12 << 16) | iter), j = t * U + u, Qk = ceil(H * U / 4), element j from word
j & 3, Box-Muller on the word pairs (0, 1), (2, 3).
"""
import numpy as np

from oracle import oracle_np as O
from tests import elite_carry_util as EC
from tests import philox_np as PH
from tests.reward_mlp_util import ACT, act_np

F = np.float32
NOISE_POLICY = 12


class PolicyNet:
    """One test policy: weights, statistics."""

    def __init__(self, name, S, U, hidden, acts, normalized, seed, out_scale=0.6):
        self.name, self.S, self.U, self.acts = name, S, U, list(acts)
        self.dims = [S] + list(hidden) + [U]
        assert len(self.acts) == len(self.dims) - 1
        rng = np.random.default_rng(seed)
        self.ws = [rng.normal(0, 1.0 / np.sqrt(k), (k, m)).astype(F) for k, m in zip(self.dims[:-1], self.dims[1:])]
        self.bs = [rng.normal(0, 0.1, (m,)).astype(F) for m in self.dims[1:]]
        self.stats = None
        if normalized:
            self.stats = [rng.normal(0, 0.2, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F),
                          rng.normal(0, 0.1, U).astype(F), rng.uniform(0.5, 1.5, U).astype(F)]
        # outputs O(out_scale): part of them inside bounds of +-1, part clipped
        y = self(rng.normal(0, 0.7, (512, S)))
        sc = out_scale / max(float(np.std(y)), 1e-3)
        self.ws[-1] = (self.ws[-1] * sc).astype(F)
        self.bs[-1] = (self.bs[-1] * sc).astype(F)

    def __call__(self, s):
        """pi on rows [B, S] -> [B, U], float64; no noise, no clip"""
        x = np.asarray(s, np.float64).reshape(-1, self.S)
        if self.stats is not None:
            x = (x - self.stats[0].astype(np.float64)) / (self.stats[1].astype(np.float64) + np.float64(F(1e-7)))
        for w, b, a in zip(self.ws, self.bs, self.acts):
            x = act_np(a, x @ w.astype(np.float64) + b.astype(np.float64))
        if self.stats is not None:
            x = x * self.stats[3].astype(np.float64) + self.stats[2].astype(np.float64)
        return x

    def codes(self):
        return [ACT[a] for a in self.acts]

    def install(self, eng, count, noise_std):
        eng.set_policy_prior_mlp(self.ws, self.bs, self.codes(), stats=self.stats, count=count, noise_std=noise_std)


def model_step64(handler, s, a):
    """The learned model's noise-free step in float64, from an oracle_np.Handler around an oracle_np.MLP:
    process_input -> Dense stack -> process_output (dev + s)."""
    s, a = np.asarray(s, np.float64), np.asarray(a, np.float64)
    eps = np.float64(F(1e-7))
    if handler.is_normalized:
        x = np.concatenate([(s - handler.mean_s.astype(np.float64)) / (handler.std_s.astype(np.float64) + eps),
                            (a - handler.mean_a.astype(np.float64)) / (handler.std_a.astype(np.float64) + eps)], axis=-1)
    else:
        x = np.concatenate([s, a], axis=-1)
    net = handler.dynamics
    for w, b, act in zip(net.weights, net.biases, net.acts):
        x = x @ w.astype(np.float64) + b.astype(np.float64)
        x = 1.0 / (1.0 + np.exp(-x)) if act == "sigmoid" else act_np(act, x)
    if handler.is_normalized:
        x = handler.mean_t.astype(np.float64) + x * (handler.std_t.astype(np.float64) + eps)
    return x + s


def policy_action64(pol, s, xi, sigma, lo, hi):
    """a = clip(pi(s) + sigma * xi, lo, hi) on rows, float64"""
    return np.clip(pol(s) + np.float64(F(sigma)) * np.asarray(xi, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64))


def policy_rollouts64(pol, handler, states, xi, sigma, lo, hi):
    """Free-running statement: states [A, S], xi [A, K, H, U] -> (actions [K, A, H, U], states [K, A, H, S]) float64."""
    A, K, H, U = xi.shape
    s = np.tile(np.asarray(states, np.float64)[None], (K, 1, 1)).reshape(K * A, -1)
    acts, sts = [], []
    for t in range(H):
        a = policy_action64(pol, s, np.asarray(xi)[:, :, t].transpose(1, 0, 2).reshape(K * A, U), sigma, lo, hi)
        s = model_step64(handler, s, a)
        acts.append(a.reshape(K, A, U))
        sts.append(s.reshape(K, A, -1))
    return np.stack(acts, axis=2), np.stack(sts, axis=2)


def policy_noise_np(seed, control_step, iteration, A, K, H, U, agent_offset=0):
    """Stream 12 as documented.  float64 [A, K, H, U]."""
    hu = H * U
    hu4 = (hu + 3) // 4 * 4                             # whole Philox blocks (Qk is the same)
    w = PH.words(seed, control_step, NOISE_POLICY, iteration, K, A, hu4, agent_offset=agent_offset)     # [K, A, hu4]
    u = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    q = u.reshape(K, A, -1, 2, 2)                       # [.., block, pair, (u1, u2)]
    r = np.sqrt(-2.0 * np.log(q[..., 0]))
    ang = 2.0 * np.pi * q[..., 1]
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=-1).reshape(K, A, -1)[:, :, :hu]
    return z.transpose(1, 0, 2).reshape(A, K, H, U)


class _PriorMixin:
    """The carry optimizers of tests/elite_carry_util.py with the K policy columns written behind the draw, in front of the
    carried columns.  `rollouts(state, xi) -> actions [K, A, H, U]` is the policy rollout (the statement above, or the
    device's own rollouts in a lock-step comparison); noise["policy"][it] is xi [A, K, H, U]."""

    def _init_prior(self, count, rollouts):
        assert count >= 1 and count + max(self.keep, self.shift) < self.N
        self.K, self.rollouts = int(count), rollouts
        self.columns = []                                   # per iteration of the last _optimize: (first column, c_i)

    def _optimize(self, state, noise, forced_elites=None):
        self._state, self._noise, self._it = state, noise, 0
        self._c_first = 0 if self.stored is None else len(self.stored)
        self.columns = []
        return super()._optimize(state, noise, forced_elites=forced_elites)

    def _candidates(self, mean, var, z):
        samples = super()._candidates(mean, var, z)
        c_i = self._c_first if self._it == 0 else self.keep
        col0 = self.N - c_i - self.K
        samples[col0:col0 + self.K] = np.asarray(self.rollouts(self._state, self._noise["policy"][self._it])).astype(F)
        self.columns.append((col0, c_i))
        self._it += 1
        return samples


class _PlainPriorCEM(_PriorMixin, EC._PlainCarryCEM):
    pass


class _CorrelatedPriorCEM(_PriorMixin, EC._CorrelatedCarryCEM):
    pass


def PriorCEM(*args, count, rollouts, keep=0, shift=0, mix=None, **kw):
    """oracle_np.CEM (keep = shift = 0, mix = None: elite_carry_util.CarryCEM without carry is that optimizer), CarryCEM or
    its correlated form, with the policy columns."""
    cem = _PlainPriorCEM(*args, **kw) if mix is None else _CorrelatedPriorCEM(*args, mix=mix, **kw)
    cem._init_carry(keep, shift)
    cem._init_prior(count, rollouts)
    return cem


# ---- the test policies ---------------------------------------------------------------------------------------------------
def small_policies(S, U):
    """widths 8, 24 (no multiple of 16) and a swish layer; normalised and raw"""
    return [PolicyNet("linear", S, U, [], [None], True, 21),
            PolicyNet("tanh8", S, U, [8], ["tanh", None], True, 22),
            PolicyNet("relu24-raw", S, U, [24], ["relu", None], False, 23),
            PolicyNet("swish24-tanh8", S, U, [24, 8], ["swish", "tanh", None], True, 24)]


def wide_policy(S, U):
    return PolicyNet("200-200", S, U, [200, 200], ["tanh", "tanh", None], True, 25)


def limits_policy(S, U):
    return PolicyNet("8x512", S, U, [512] * 7, ["tanh"] * 7 + [None], True, 26)
