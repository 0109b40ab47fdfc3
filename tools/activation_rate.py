#!/usr/bin/env python
"""What each Dense activation costs in the learned-model rollout kernel (run on a GPU box).  For every activation the
rollout kernel's mean time per launch (HIP events, Engine.get_profile) at three shapes:
  cfg4      26-200-200-20, N = 1000, H = 30, cheetah reward   (k_rollout_mlp_q4s; run-time activations except tanh / relu)
  cfg_tut2  26-500-500-500-20, N = 4048, H = 15, cheetah      (generic k_rollout_mlp<0>)
  pendulum  4-32-32-3, N = 1000, H = 30, pendulum reward      (k_rollout_mlp_w4)
Every hidden layer takes the activation, the last layer none.  tanh runs the compile-time instantiations where the
dispatcher has them (q4s, w4); "sigmoid" is the run-time path the new activations share.
Usage: python tools/activation_rate.py [--out table.md] [--launches 20]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACTS = ["tanh", "sigmoid", "elu", "selu", "softplus", "softsign", "exponential", "hard_sigmoid", "swish", "leaky_relu",
        "relu6"]
SHAPES = [("cfg4", [26, 200, 200, 20], 1000, 30, "cheetah"),
          ("cfg_tut2", [26, 500, 500, 500, 20], 4048, 15, "cheetah"),
          ("pendulum", [4, 32, 32, 3], 1000, 30, "pendulum")]


def kernel_us(L, Engine, SY, act, dims, N, H, reward, launches):
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    S, U = dims[-1], dims[0] - dims[-1]
    codes = DeterministicMLP(dims, [act] * (len(dims) - 2) + [None]).activation_codes
    rk = L.REW_CHEETAH if reward == "cheetah" else L.REW_PENDULUM
    lim = 2.0 if reward == "pendulum" else 1.0
    eng = Engine(L.OPT_NONE, L.DYN_MLP, rk, [-lim] * U, [lim] * U, dim_s=S, num_agents=1, planning_horizon=H)
    eng.set_mlp(*SY.make_mlp_params(dims), codes, SY.cheetah_stats(S, U) if reward == "cheetah" else None)
    start = SY.cheetah_start_states(1, S) if reward == "cheetah" else SY.pendulum_start_states(1)
    seq = np.random.default_rng(0).uniform(-lim, lim, (N, 1, H, U)).astype(np.float32)
    for _ in range(3):
        eng.evaluate(start, seq)
    eng.synchronize()
    eng.set_profiling(True)
    for _ in range(launches):
        eng.evaluate(start, seq)
    eng.synchronize()
    ms, n, _ = eng.get_profile()
    inst = eng.profile_instantiation()
    eng.set_profiling(False)
    return ms * 1e3 / n, inst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--acts", default=",".join(ACTS), help="comma-separated subset (tanh,sigmoid runs on any version)")
    args = ap.parse_args()
    acts = args.acts.split(",")
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.utils import synthetic as SY
    res = {}
    for act in acts:
        for name, dims, N, H, reward in SHAPES:
            res[act, name] = kernel_us(L, Engine, SY, act, dims, N, H, reward, args.launches)
    head = "| activation | " + " | ".join("%s us (kernel)" % s[0] for s in SHAPES) + " |"
    lines = [head, "|---|" + "---:|" * len(SHAPES)]
    for act in acts:
        lines.append("| %s | " % act + " | ".join("%.1f (%s)" % res[act, s[0]] for s in SHAPES) + " |")
    base = {s[0]: res["sigmoid", s[0]][0] for s in SHAPES}
    lines += ["", "relative to run-time sigmoid at the same shape:", "",
              "| activation | " + " | ".join(s[0] for s in SHAPES) + " |", "|---|" + "---:|" * len(SHAPES)]
    for act in acts:
        lines.append("| %s | " % act + " | ".join("%.3f" % (res[act, s[0]][0] / base[s[0]]) for s in SHAPES) + " |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
