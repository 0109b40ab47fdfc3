"""Learned terminal values (bbmpc_set_terminal_value_mlp): the float64 NumPy statement, the test networks and the HIP-source
twin that tests/test_terminal_value_cpu.py and tests/test_gpu_terminal_value.py share.  Test infrastructure only.

The statement, for a value network over the state alone -- Dense layers (W_l [in, out], b_l, act_l)
ending in one output, statistics (mean_in [S], std_in [S], mean_v, std_v) or none:
    x = (s - mean_in) / (std_in + float32(1e-7))                       (skipped without statistics)
    for every layer: x = act_l(x W_l + b_l)
    V(s) = x[0] * std_v + mean_v                                       (V = x[0] without statistics)
    R'[n, a] = R[n, a] + w * V(s_H[n, a]);   w * V NaN -> R' = -1e6
where R is the handle's score without the network and s_H the state after the rollout's last step.

A value network is tests/reward_mlp_util.Net with mask 1 (s_t alone)."""
import numpy as np

from tests import reward_mlp_util as R

F = np.float32


def value(net, states):
    """V on rows [B, S] -> [B] float64"""
    return net.raw(np.asarray(states, np.float64).reshape(-1, net.S))


def with_terminal(base, net, weight, s_last):
    """base [N, A] (the handle's scores without the network), s_last [N, A, S] -> R' [N, A] float64"""
    base = np.asarray(base, np.float64)
    term = np.float64(weight) * value(net, np.asarray(s_last).reshape(-1, net.S)).reshape(base.shape)
    return np.where(np.isnan(term), -1.0e6, base + term)


# ---- the test networks over S = 3 (a multiple of neither 4 nor 16), hidden widths 20 and 33 ----------------------------
def small_nets():
    return [R.Net("v-linear", 3, 1, 1, [], [None], True, 21),
            R.Net("v-tanh20", 3, 1, 1, [20], ["tanh", None], True, 22),
            R.Net("v-tanh20-raw", 3, 1, 1, [20], ["tanh", None], False, 23),
            R.Net("v-relu33-raw", 3, 1, 1, [33], ["relu", None], False, 24),
            R.Net("v-swish20-tanh33", 3, 1, 1, [20, 33], ["swish", "tanh", None], True, 25)]


def medium_net():
    return R.Net("v-20-200-200-1", 20, 6, 1, [200, 200], ["tanh", "tanh", None], True, 26)


def limits_net():
    return R.Net("v-64-7x512-1", 64, 64, 1, [512] * 7, ["tanh"] * 7 + [None], True, 27)


# ---- the HIP-source twin: reward network at every step + w * V(nxt) at the last one, weights as runtime parameters ----------
def _net_params(net):
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in zip(net.ws, net.bs)] +
                          ([np.concatenate(net.stats)] if net.stats is not None else [])).astype(F)


def _net_lines(net, base, result):
    """Source lines that run `net` on x[0 .. D) (already assembled) with its parameters at p[base ...] and leave the
    de-normalised output in the float variable `result`.  Layout as reward_mlp_util.twin_source_and_params."""
    off = base + sum(w.size + b.size for w, b in zip(net.ws, net.bs))
    lines = []
    if net.stats is not None:
        lines.append("    for (int i = 0; i < %d; ++i) x[i] = (x[i] - p[%d + i]) / (p[%d + i] + 1e-7f);" % (net.D, off, off + net.D))
    o = base
    for (w, b, a) in zip(net.ws, net.bs, net.acts):
        K, M = w.shape
        lines += ["    for (int j = 0; j < %d; ++j) {" % M,
                  "        float v = p[%d + j];" % (o + K * M),
                  "        for (int i = 0; i < %d; ++i) v = v + x[i] * p[%d + i * %d + j];" % (K, o, M),
                  "        y[j] = %s;" % R._ACT_SRC[a], "    }",
                  "    for (int j = 0; j < %d; ++j) x[j] = y[j];" % M]
        o += K * M + M
    lines.append("    %s = x[0] * p[%d] + p[%d];" % (result, off + 2 * net.D + 1, off + 2 * net.D) if net.stats is not None
                 else "    %s = x[0];" % result)
    return lines


def twin_source_and_params(reward_net, value_net, weight, H):
    """(HIP source of bbmpc_user_reward_params, params [P]): r(cur, act, nxt) of `reward_net` at every step, plus
    weight * V(nxt) of `value_net` when t == H - 1.  params = reward network | value network | weight."""
    pr, pv = _net_params(reward_net), _net_params(value_net)
    params = np.concatenate([pr, pv, np.array([weight], F)]).astype(F)
    assert params.size <= 4096
    wmax = max(max(reward_net.dims), max(value_net.dims))
    lines = ["__device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,",
             "                                          const float* p, int t) {",
             "    float x[%d], y[%d], r, val;" % (wmax, wmax), "    int k = 0;"]
    if reward_net.mask & 1:
        lines.append("    for (int i = 0; i < %d; ++i) x[k++] = cur[i];" % reward_net.S)
    if reward_net.mask & 2:
        lines.append("    for (int i = 0; i < %d; ++i) x[k++] = act[i];" % reward_net.U)
    if reward_net.mask & 4:
        lines.append("    for (int i = 0; i < %d; ++i) x[k++] = nxt[i];" % reward_net.S)
    lines += _net_lines(reward_net, 0, "r")
    lines.append("    if (t != %d) return r;" % (H - 1))
    lines.append("    for (int i = 0; i < %d; ++i) x[i] = nxt[i];" % value_net.S)
    lines += _net_lines(value_net, pr.size, "val")
    lines.append("    return r + p[%d] * val;" % (pr.size + pv.size))
    lines.append("}")
    return "\n".join(lines) + "\n", params
