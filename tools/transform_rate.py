#!/usr/bin/env python
"""What a custom inverse target transform costs (run on a GPU box).  Config 4's size: the 26-200-200-20 tanh HalfCheetah
MLP, cheetah reward, CEM N=1000 H=30 5 iterations, 1 agent.  us per control step (optimize_dev, device in / device out)
and the dominant kernel's mean time per launch (HIP events) for
  1. the built-in path,
  2. the same forced to the generic MFMA kernel (BBMPC_MLP_GENERIC=1, k_rollout_mlp<0>),
  3. a HIP transform equal to the default (next = state + dev), fused into the learned-model rollout (hiprtc),
  4. the same transform step-wise (BBMPC_USER_STEPWISE=1).
Usage: python tools/transform_rate.py [--out table.md]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_XFORM = """
__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {
    for (int i = 0; i < S; ++i) next[i] = cur[i] + dev[i];
}
"""


def rate(eng, start, steps, rec_width):
    import torch
    dev = torch.device("cuda", 0)
    st = torch.from_numpy(start).to(dev)
    nx = torch.empty_like(st)
    rec = torch.zeros((start.shape[0], rec_width), device=dev)
    for _ in range(5):
        eng.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
        st, nx = nx, st
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
        st, nx = nx, st
    eng.synchronize()
    us = (time.perf_counter() - t0) / steps * 1e6
    # the dominant kernel alone, events around every launch (a separate pass: the events cost host time)
    eng.set_profiling(True)
    for _ in range(3):
        eng.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
        st, nx = nx, st
    eng.synchronize()
    ms, launches, name = eng.get_profile()
    eng.set_profiling(False)
    return us, (ms * 1e3 / launches if launches else float("nan")), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.utils import synthetic as SY
    S, U = 20, 6
    kw = dict(dim_s=S, num_agents=1, planning_horizon=30, population_size=1000, max_iterations=5, num_elite=50)
    start = SY.cheetah_start_states(1)

    def engine(env, xform):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            e = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_CHEETAH, [-1.0] * U, [1.0] * U, **kw)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        e.set_mlp(*SY.make_mlp_params(), [1, 1, 0], SY.cheetah_stats(S, U))
        if xform:
            e.set_inverse_transform_source(DEFAULT_XFORM)
        e.reset()
        return e

    rows = [("built-in path", {}, False, 100),
            ("built-in, generic kernel (BBMPC_MLP_GENERIC=1)", {"BBMPC_MLP_GENERIC": "1"}, False, 100),
            ("HIP transform (= default), fused", {}, True, 100),
            ("HIP transform (= default), step-wise (BBMPC_USER_STEPWISE=1)", {"BBMPC_USER_STEPWISE": "1"}, True, 20)]
    lines = ["| path | us / control step | dominant kernel | us / launch |", "|---|---:|---|---:|"]
    for name, env, xform, steps in rows:
        us, k_us, kname = rate(engine(env, xform), start, steps, U + S + 1)
        lines.append("| %s | %.1f | %s | %.1f |" % (name, us, kname, k_us))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
