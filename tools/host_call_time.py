"""Wall time per call of two host-in / host-out entry points, for comparing two builds of the library:

    python tools/host_call_time.py [--tree DIR] [--calls 2000] [--warmup 200]

bbmpc_predict_next_state at batch 1 and bbmpc_predict_trajectories at batch 70, Hq = 3, on a learned-model handle
(S = 3, U = 1, 4-24-3 network, A = 2): the median over --calls calls after --warmup calls, each timed with
time.perf_counter_ns around the ctypes call (buffers and pointers prepared once).  --tree: import the package from that
checkout instead of this one (its library must be built).  Prints one JSON line.  profiles/host_stage.md has the figures
of the change that introduced HostStage against its parent."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    F = np.float32
    S, U, A, H = 3, 1, 2, 3
    rng = np.random.default_rng(0)
    dims = [S + U, 24, S]
    ws = [rng.normal(0, 0.3, (dims[i], dims[i + 1])).astype(F) for i in range(2)]
    bs = [rng.normal(0, 0.1, dims[i + 1]).astype(F) for i in range(2)]
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-1.0], [1.0], dim_s=S, num_agents=A, planning_horizon=H)
    eng.set_mlp(ws, bs, [1, 0])

    def timed(call):
        for _ in range(args.warmup):
            assert call() == 0
        t = np.empty(args.calls, np.int64)
        for i in range(args.calls):
            t0 = time.perf_counter_ns()
            call()
            t[i] = time.perf_counter_ns() - t0
        return {"median_us": float(np.median(t)) / 1e3, "p10_us": float(np.percentile(t, 10)) / 1e3, "p90_us": float(np.percentile(t, 90)) / 1e3}

    s1, a1, n1 = rng.normal(0, 0.5, (1, S)).astype(F), rng.uniform(-1, 1, (1, U)).astype(F), np.empty((1, S), F)
    p1 = (L.ptr(s1), L.ptr(a1), L.ptr(n1))
    B = 70
    sb, qb = rng.normal(0, 0.5, (B, S)).astype(F), rng.uniform(-1, 1, (B, H, U)).astype(F)
    ob, rb = np.empty((B, H, S), F), np.empty((B, H), F)
    pb = (L.ptr(sb), L.ptr(qb), L.ptr(ob), L.ptr(rb))
    out = {"tree": os.path.abspath(args.tree), "calls": args.calls, "warmup": args.warmup,
           "predict_next_state_b1": timed(lambda: L.lib.bbmpc_predict_next_state(eng._h, p1[0], p1[1], 1, p1[2])),
           "predict_trajectories_b70_h3": timed(lambda: L.lib.bbmpc_predict_trajectories(eng._h, pb[0], pb[1], B, H, pb[2], pb[3]))}
    assert np.all(np.isfinite(n1)) and np.all(np.isfinite(ob)) and np.all(np.isfinite(rb))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
