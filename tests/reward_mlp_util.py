"""Learned reward models (BBMPC_REW_MLP): the float64 NumPy statement of the scorer, the test networks and the HIP-source
twin that tests/test_reward_mlp_cpu.py (statement alone) and tests/test_gpu_reward_mlp.py (device against statement and
against the existing HIP-source path) share.  Test infrastructure only.

The statement, for a network with input_mask m (bit 0 s_t, bit 1 a_t, bit 2 s_{t+1}), Dense layers (W_l [in, out], b_l, act_l)
ending in one output and statistics (mean_in, std_in, mean_r, std_r) or none:
    x = concat of the selected blocks in the order s_t, a_t, s_{t+1}
    x = (x - mean_in) / (std_in + float32(1e-7))                      (bbmpc_process_input's rule; skipped without statistics)
    for every layer: x = act_l(x W_l + b_l)
    r = x[0] * std_r + mean_r                                          (r = x[0] without statistics)
    R[n, a] = sum over t ascending of r(s_t, a_t, s_{t+1});  NaN -> -1e6;  R - penalty where a bound penalty applies
"""
import numpy as np

F = np.float32
ACT = {None: 0, "tanh": 1, "relu": 2, "swish": 10}
ONE_STEP = (2e-5, 2e-5)                 # rtol, atol of tests/test_gpu_mlp.py's single model step
H_STEP_RTOL, H_STEP_ATOL_PER_STEP = 1e-3, 1e-3      # ... and of its H-step rewards: rtol 1e-3 + atol 1e-3 * H


def act_np(name, x):
    if name == "tanh":
        return np.tanh(x)
    if name == "relu":
        return np.maximum(x, 0.0)
    if name == "swish":
        return x / (1.0 + np.exp(-x))
    assert name is None, name
    return x


class Net:
    """One test network: weights, statistics, mask."""

    def __init__(self, name, S, U, mask, hidden, acts, normalized, seed):
        self.name, self.S, self.U, self.mask, self.acts = name, S, U, mask, list(acts)
        self.D = (S if mask & 1 else 0) + (U if mask & 2 else 0) + (S if mask & 4 else 0)
        self.dims = [self.D] + list(hidden) + [1]
        assert len(self.acts) == len(self.dims) - 1
        rng = np.random.default_rng(seed)
        self.ws = [rng.normal(0, 1.0 / np.sqrt(k), (k, m)).astype(F) for k, m in zip(self.dims[:-1], self.dims[1:])]
        self.bs = [rng.normal(0, 0.1, (m,)).astype(F) for m in self.dims[1:]]
        self.stats = None
        if normalized:
            self.stats = [rng.normal(0, 0.2, self.D).astype(F), rng.uniform(0.5, 1.5, self.D).astype(F),
                          np.array([0.3], F), np.array([1.7], F)]
        # outputs O(1): the last layer is scaled so that the raw output has unit spread on standard-normal-sized inputs
        y = self.raw(rng.normal(0, 0.7, (512, self.D)))
        sc = 1.0 / max(float(np.std(y)), 1e-3)
        self.ws[-1] = (self.ws[-1] * sc).astype(F)
        self.bs[-1] = (self.bs[-1] * sc).astype(F)

    def raw(self, x, ws=None, bs=None):
        """normalise -> Dense stack -> de-normalise on assembled rows [B, D], float64"""
        ws, bs = ws or self.ws, bs or self.bs
        x = np.asarray(x, np.float64)
        if self.stats is not None:
            x = (x - self.stats[0].astype(np.float64)) / (self.stats[1].astype(np.float64) + np.float64(F(1e-7)))
        for w, b, a in zip(ws, bs, self.acts):
            x = act_np(a, x @ w.astype(np.float64) + b.astype(np.float64))
        y = x[:, 0]
        if self.stats is not None:
            y = y * np.float64(self.stats[3][0]) + np.float64(self.stats[2][0])
        return y

    def assemble(self, cur, act, nxt):
        blocks = []
        if self.mask & 1:
            blocks.append(np.asarray(cur, np.float64).reshape(-1, self.S))
        if self.mask & 2:
            blocks.append(np.asarray(act, np.float64).reshape(-1, self.U))
        if self.mask & 4:
            blocks.append(np.asarray(nxt, np.float64).reshape(-1, self.S))
        return np.concatenate(blocks, 1)

    def rows(self, cur, act, nxt, **kw):
        """r(s_t, a_t, s_{t+1}) on rows -> [B] float64"""
        return self.raw(self.assemble(cur, act, nxt), **kw)

    def n_params(self):
        return sum(w.size + b.size for w, b in zip(self.ws, self.bs)) + (2 * self.D + 2 if self.stats is not None else 0)

    def codes(self):
        return [ACT[a] for a in self.acts]


def per_step(net, start, states, actions, **kw):
    """start [B, S], states [B, Hq, S] (the state AFTER every step), actions [B, Hq, U] -> rewards [B, Hq] float64"""
    B, Hq = actions.shape[0], actions.shape[1]
    cur = np.concatenate([np.asarray(start)[:, None], np.asarray(states)[:, :-1]], 1)
    return net.rows(cur.reshape(B * Hq, -1), np.asarray(actions).reshape(B * Hq, -1), np.asarray(states).reshape(B * Hq, -1), **kw).reshape(B, Hq)


def returns(step_rewards):
    """[..., H] per-step rewards -> the evaluator's sum over t ascending with NaN -> -1e6"""
    total = np.zeros(step_rewards.shape[:-1], np.float64)
    for t in range(step_rewards.shape[-1]):
        total = total + step_rewards[..., t]
    return np.where(np.isnan(total), -1.0e6, total)


# ---- the test networks: S = 3, U = 1 (D = 7: a multiple of neither 4 nor 16), hidden widths 20 and 33 -----------------
def small_nets():
    return [Net("linear-sas", 3, 1, 7, [], [None], True, 11),
            Net("tanh20-sas", 3, 1, 7, [20], ["tanh", None], True, 12),
            Net("tanh20-sas-raw", 3, 1, 7, [20], ["tanh", None], False, 13),
            Net("relu33-sa", 3, 1, 3, [33], ["relu", None], False, 14),
            Net("swish20-tanh33-next", 3, 1, 4, [20, 33], ["swish", "tanh", None], True, 15)]


def medium_net():
    return Net("46-200-200-1", 20, 6, 7, [200, 200], ["tanh", "tanh", None], True, 16)


def limits_net():
    return Net("192-8x512", 64, 64, 7, [512] * 7, ["tanh"] * 7 + [None], True, 17)


# ---- the HIP-source twin: the same network as a HipRewardFunction with its weights as runtime parameters ----------------
_ACT_SRC = {None: "v", "tanh": "tanhf(v)", "relu": "fmaxf(v, 0.0f)", "swish": "v / (1.0f + expf(-v))"}


def twin_source_and_params(net):
    """(HIP source of bbmpc_user_reward_params, params [P]): layers as (W row-major [in][out], b) one after the other, then
    mean_in, std_in, mean_r, std_r when normalised."""
    assert net.n_params() <= 4096
    params = np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in zip(net.ws, net.bs)] +
                            ([np.concatenate(net.stats)] if net.stats is not None else [])).astype(F)
    wmax = max(net.dims)
    lines = ["__device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,",
             "                                          const float* p, int t) {",
             "    float x[%d], y[%d];" % (wmax, wmax), "    int k = 0;"]
    if net.mask & 1:
        lines.append("    for (int i = 0; i < %d; ++i) x[k++] = cur[i];" % net.S)
    if net.mask & 2:
        lines.append("    for (int i = 0; i < %d; ++i) x[k++] = act[i];" % net.U)
    if net.mask & 4:
        lines.append("    for (int i = 0; i < %d; ++i) x[k++] = nxt[i];" % net.S)
    off = sum(w.size + b.size for w, b in zip(net.ws, net.bs))
    if net.stats is not None:
        lines.append("    for (int i = 0; i < %d; ++i) x[i] = (x[i] - p[%d + i]) / (p[%d + i] + 1e-7f);" % (net.D, off, off + net.D))
    o = 0
    for (w, b, a) in zip(net.ws, net.bs, net.acts):
        K, M = w.shape
        lines += ["    for (int j = 0; j < %d; ++j) {" % M,
                  "        float v = p[%d + j];" % (o + K * M),
                  "        for (int i = 0; i < %d; ++i) v = v + x[i] * p[%d + i * %d + j];" % (K, o, M),
                  "        y[j] = %s;" % _ACT_SRC[a], "    }",
                  "    for (int j = 0; j < %d; ++j) x[j] = y[j];" % M]
        o += K * M + M
    lines.append("    return x[0] * p[%d] + p[%d];" % (off + 2 * net.D + 1, off + 2 * net.D) if net.stats is not None else "    return x[0];")
    lines.append("}")
    return "\n".join(lines) + "\n", params


# ---- data: states of a "trajectory" for the statement-only tests -----------------------------------------------------------
def random_trajectories(net, B, Hq, seed, lo=None, hi=None):
    """start [B, S], states [B, Hq, S], raw actions [B, Hq, U] (partly outside [lo, hi] when bounds are given)"""
    rng = np.random.default_rng(seed)
    start = rng.normal(0, 0.7, (B, net.S))
    states = start[:, None] + np.cumsum(rng.normal(0, 0.5, (B, Hq, net.S)), 1)
    if lo is None:
        actions = rng.uniform(-1, 1, (B, Hq, net.U))
    else:
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        actions = rng.uniform(lo - 3 * (hi - lo), hi + 3 * (hi - lo), (B, Hq, net.U))
    return start, states, actions
