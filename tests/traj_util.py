"""Yardsticks for the open-loop trajectory tests: the oracle's one-step calls composed Hq times (float32, oracle/oracle_np.py
as it is) and a float64 evaluation of the same recurrence (weights and inputs cast up), plus the cases both GPU and CPU
runs use.

The bound of tests/test_gpu_predict_trajectories.py: at every step t the device's deviation from the float64 evaluation
may be at most FACTOR x the float32 oracle's own maximum deviation from float64 at that t, plus the one-step tolerance
(rtol 2e-5, atol 2e-5 of tests/test_gpu_mlp.py for states; rtol 1e-4, atol 1e-3 for rewards).  FACTOR = 4 allows for a
different K-summation order and the hardware tanh / exp forms (1e-6 relative each); it is not a measured value."""
import numpy as np

from oracle import oracle_np as O

F = np.float32
FACTOR = 4.0
STATE_RTOL, STATE_ATOL = 2e-5, 2e-5
REWARD_RTOL, REWARD_ATOL = 1e-4, 1e-3


def oracle_trajectories(ev, states, seq):
    """Evaluator.predict_next_state / evaluate_next_reward composed Hq times: states [B,S], seq [B,Hq,U] ->
    (states [B,Hq,S], rewards [B,Hq]) float32."""
    s = np.asarray(states, F)
    seq = np.asarray(seq, F)
    out_s, out_r = [], []
    for t in range(seq.shape[1]):
        nxt = ev.predict_next_state(s, seq[:, t])
        out_r.append(ev.evaluate_next_reward(s, nxt, seq[:, t]))
        out_s.append(nxt)
        s = nxt
    return np.stack(out_s, 1), np.stack(out_r, 1)


# ---- float64 forms ------------------------------------------------------------------------------------------------------
def _act64(name, x):
    if name is None:
        return x
    if name == "tanh":
        return np.tanh(x)
    if name == "relu":
        return np.maximum(x, 0.0)
    if name == "sigmoid":
        return 0.5 * (1.0 + np.tanh(0.5 * x))
    if name == "swish":
        return x * 0.5 * (1.0 + np.tanh(0.5 * x))
    raise ValueError(name)


def pendulum_reward64(cur, nxt, act, as_executed=True):
    th = np.arctan2(cur[:, 1], cur[:, 0])
    ang = np.mod(th + np.pi, 2 * np.pi) - np.pi
    src = nxt if as_executed else act
    return -(ang * ang + 0.1 * cur[:, 2] ** 2) - 0.001 * np.sum(src * src, axis=1)


def pendulum_step64(s, u):
    th = np.arctan2(s[:, 1], s[:, 0])
    acc = -15.0 * np.sin(th + np.pi) + 3.0 * u[:, 0]
    nthd = s[:, 2] + acc * 0.05
    nth = th + nthd * 0.05
    nthd = np.clip(nthd, -8.0, 8.0)
    return np.stack([np.cos(nth), np.sin(nth), nthd], 1)


class Mlp64:
    """process_input -> Dense stack -> process_output (system_dynamics_handler.py:97-161) in float64."""

    def __init__(self, ws, bs, acts, stats=None):
        self.ws = [np.asarray(w, np.float64) for w in ws]
        self.bs = [np.asarray(b, np.float64) for b in bs]
        self.acts = list(acts)
        # the constants as the float32 code forms them (std + 1e-7 rounded to float32), then cast up: inputs cast up
        self.stats = None if stats is None else [np.asarray(v, F) for v in stats]

    def __call__(self, s, u):
        if self.stats is not None:
            ms, ss, ma, sa, mt, st = self.stats
            x = np.concatenate([(s - ms.astype(np.float64)) / (ss + F(1e-7)).astype(np.float64),
                                (u - ma.astype(np.float64)) / (sa + F(1e-7)).astype(np.float64)], 1)
        else:
            x = np.concatenate([s, u], 1)
        for w, b, a in zip(self.ws, self.bs, self.acts):
            x = _act64(a, x @ w + b)
        if self.stats is not None:
            x = mt.astype(np.float64) + x * (st + F(1e-7)).astype(np.float64)
        return x + s


def trajectories64(step, states, seq, as_executed=True):
    """The recurrence in float64 with the pendulum reward: (states [B,Hq,S], rewards [B,Hq])."""
    s = np.asarray(states, np.float64)
    seq = np.asarray(seq, np.float64)
    out_s, out_r = [], []
    for t in range(seq.shape[1]):
        nxt = step(s, seq[:, t])
        out_r.append(pendulum_reward64(s, nxt, seq[:, t], as_executed))
        out_s.append(nxt)
        s = nxt
    return np.stack(out_s, 1), np.stack(out_r, 1)


def stats_for(S, U, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 0.2, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F),
            rng.normal(0, 0.1, U).astype(F), rng.uniform(0.5, 1.5, U).astype(F),
            rng.normal(0, 0.01, S).astype(F), rng.uniform(0.05, 0.15, S).astype(F)]


# name -> (dims, activations, normalised, B, Hq); every learned case scores with the pendulum reward (continuous in the
# state, unlike the cheetah reward's thresholds), networks from oracle_np.make_mlp_params (last-layer scale 0.1)
MLP_CASES = {
    "mlp200_norm_B4099_H50": ([26, 200, 200, 20], ["tanh", "tanh", None], True, 4099, 50),
    "mlp200_raw_B77_H30": ([26, 200, 200, 20], ["tanh", "tanh", None], False, 77, 30),
    "mlp500x3_norm_B77_H50": ([26, 500, 500, 500, 20], ["tanh", "tanh", "tanh", None], True, 77, 50),
    "mlp32_norm_B1_H50": ([26, 32, 32, 20], ["tanh", "tanh", None], True, 1, 50),
    "mlp200_swish_B77_H30": ([26, 200, 200, 20], ["swish", "swish", None], True, 77, 30),
    "mlp64_S17U6_B77_H30": ([23, 64, 64, 17], ["tanh", "relu", None], True, 77, 30),
    "mlp64_S17U6_B16_H1": ([23, 64, 64, 17], ["tanh", "relu", None], False, 16, 1),
}
PENDULUM_CASES = {"pendulum_B77_H50": (77, 50), "pendulum_B4099_H30": (4099, 30), "pendulum_B1_H1": (1, 1)}


def mlp_case(name):
    """-> dict(ws, bs, acts, stats, states, seq, S, U)"""
    dims, acts, normd, B, Hq = MLP_CASES[name]
    S = dims[-1]
    U = dims[0] - S
    ws, bs = O.make_mlp_params(dims, seed=42)
    rng = np.random.default_rng(sum(map(ord, name)))
    bs = [rng.normal(0, 0.05, b.shape).astype(F) for b in bs]
    stats = stats_for(S, U, 5) if normd else None
    states = (rng.standard_normal((B, S)) * 0.3).astype(F)
    states[:, 0] += F(1.0)                         # the pendulum reward's atan2(s1, s0) stays away from the origin
    seq = rng.uniform(-1, 1, (B, Hq, U)).astype(F)
    return dict(ws=ws, bs=bs, acts=acts, stats=stats, states=states, seq=seq, S=S, U=U)


def pendulum_case(name):
    B, Hq = PENDULUM_CASES[name]
    states = O.pendulum_start_states(B)
    seq = np.random.default_rng(B * 1000 + Hq).uniform(-2, 2, (B, Hq, 1)).astype(F)
    return dict(states=states, seq=seq)


def oracle_mlp_evaluator(c):
    if "swish" in c["acts"]:
        from tests.test_gpu_activations import MLP64 as OracleMlp     # the oracle's Dense stack with the TF 2.0 swish
    else:
        OracleMlp = O.MLP
    h = O.Handler(OracleMlp(c["ws"], c["bs"], c["acts"]), False, c["stats"] is not None, c["stats"])
    return O.Evaluator("pendulum", h)


def per_step_dev(x, ref64):
    """max |x - ref64| per step: [B,Hq,...] -> [Hq]"""
    d = np.abs(np.asarray(x, np.float64) - ref64)
    return d.reshape(d.shape[0], d.shape[1], -1).max(axis=(0, 2))


def check_against_float64(got, oracle32, ref64, rtol, atol, what):
    """Every element of `got` within FACTOR x the oracle's per-step maximum deviation from float64, plus the one-step
    tolerance; prints the measured ratio per step first.  Returns the largest ratio (device deviation / oracle deviation)."""
    dev_o = per_step_dev(oracle32, ref64)
    dev_g = per_step_dev(got, ref64)
    ratio = dev_g / np.maximum(dev_o, 1e-30)
    print("%s: oracle dev t=last %.3e, device dev t=last %.3e, max ratio %.2f (steps %s)"
          % (what, dev_o[-1], dev_g[-1], ratio.max(), np.array2string(ratio[:: max(1, len(ratio) // 10)], precision=2)))
    shape = [1, -1] + [1] * (ref64.ndim - 2)
    bound = FACTOR * dev_o.reshape(shape) + atol + rtol * np.abs(ref64)
    err = np.abs(np.asarray(got, np.float64) - ref64)
    bad = err > bound
    assert not bad.any(), ("%s: %d elements outside %g x the oracle's deviation + tolerance; worst excess %.3e at %s"
                           % (what, int(bad.sum()), FACTOR, float((err - bound).max()),
                              np.unravel_index(np.argmax(err - bound), err.shape)))
    return float(ratio.max())
