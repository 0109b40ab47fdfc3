"""What a plan gradient (bbmpc_plan_gradient, k_plan_grad) costs beside the forward-only path, and what refinement costs and
buys.  Prints markdown; the committed copy is profiles/plan_gradient.md.

    python tools/plan_gradient_rate.py > profiles/plan_gradient.md

Method.  Every comparison alternates its legs (A B A B ...), `rounds` times; a leg is the median of `reps` timed calls
after a warm-up, and the table gives the median of the leg medians with their min .. max as the spread.
 * Gradient against forward only: B = 1000 rows, Hq = 30, 26-200-200-20 dynamics, 46-200-200-1 reward network, 20-200-200-1
   value network, device pointers, stream events on the handle's torch stream.  The forward-only leg is what the handle
   had before: predict_trajectories_dev (states and per-step rewards: k_traj_mlp + k_reward_mlp_rows) followed by
   evaluate_terminal_value_dev on the last states (gathered by one strided torch copy, inside the timed window).
 * Control step: host-in / host-out MPCPolicy-style step (wall clock): Engine.optimize of a CEM handle (N = 1000, 5
   iterations, H = 30) with plan readback on, alone and followed by refine_plan(steps = 3) on its plan (4 gradient calls
   of one row, host arrays).
 * Closed-loop returns: examples/plan_gradient_pendulum.py's setup, the same start states for every leg."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
F = np.float32


def _params(dims, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0, 1 / np.sqrt(k), (k, m)).astype(F) for k, m in zip(dims[:-1], dims[1:])]
    return ws, [rng.normal(0, 0.05, (m,)).astype(F) for m in dims[1:]]


def _alternate(legs, rounds):
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(fn())
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in got.items()}


def _fmt(t):
    return "%.1f (%.1f .. %.1f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)


def main(reps=40, rounds=5, closed_loop=True):
    import torch
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan
    stream = torch.cuda.Stream()
    S, U, B, H = 20, 6, 1000, 30
    acts = [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE]
    lines = ["# Plan gradients: measured cost and effect", "",
             "Produced by `tools/plan_gradient_rate.py` on %s; its docstring states the method.  Times are medians over %d"
             % (torch.cuda.get_device_name(0), rounds),
             "alternating rounds of %d-call medians, spread = min .. max of the round medians." % reps, ""]

    def handle(opt=L.OPT_NONE, **kw):
        eng = Engine(opt, L.DYN_MLP, L.REW_MLP, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=1, planning_horizon=H, **kw)
        ws, bs = _params([26, 200, 200, 20], 1)
        ws[-1] *= F(0.05)
        eng.set_mlp(ws, bs, acts, None)
        eng.set_reward_mlp(*_params([46, 200, 200, 1], 3), acts, 7, None)
        eng.set_terminal_value_mlp(*_params([20, 200, 200, 1], 2), acts, None, 1.0)
        return eng

    eng = handle()
    eng.set_torch_stream(stream)
    st = (torch.rand((B, S), device="cuda") - 0.5).contiguous()
    seq = (torch.rand((B, H, U), device="cuda") * 2 - 1).contiguous()
    ret, grad = torch.empty((B,), device="cuda"), torch.empty((B, H, U), device="cuda")
    so, ro, last, val = torch.empty((B, H, S), device="cuda"), torch.empty((B, H), device="cuda"), torch.empty((B, S), device="cuda"), torch.empty((B,), device="cuda")
    torch.cuda.synchronize()

    def gradient():
        eng.plan_gradient_dev(st.data_ptr(), seq.data_ptr(), B, H, ret.data_ptr(), grad.data_ptr())

    def forward_only():
        eng.predict_trajectories_dev(st.data_ptr(), seq.data_ptr(), B, H, so.data_ptr(), ro.data_ptr())
        with torch.cuda.stream(stream):
            last.copy_(so[:, -1])
        eng.evaluate_terminal_value_dev(last.data_ptr(), B, val.data_ptr())

    def timed(fn):
        def leg():
            for _ in range(5):
                fn()
            stream.synchronize()
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                ts.append(a.elapsed_time(b))
            return float(np.median(ts))
        return leg
    ev = _alternate({"forward": timed(forward_only), "gradient": timed(gradient)}, rounds)
    lines += ["## One call, B = 1000 rows, Hq = 30, 26-200-200-20 dynamics + 46-200-200-1 reward + 20-200-200-1 value (63 workgroups of 13 waves)", "",
              "| call | time [us] |", "|---|---|",
              "| forward only: predict_trajectories_dev + last-state copy + evaluate_terminal_value_dev | %s |" % _fmt(ev["forward"]),
              "| plan_gradient_dev (returns and gradient, one launch of k_plan_grad) | %s |" % _fmt(ev["gradient"]),
              "| ratio of the medians, gradient / forward only | %.2f |" % (ev["gradient"][0] / ev["forward"][0]), ""]

    # ---- control step with and without refinement ----------------------------------------------------------------------------
    cem = handle(opt=L.OPT_CEM, population_size=1000, max_iterations=5, num_elite=100, seed=1)
    cem.set_keep_plan(True)
    state = np.full((1, S), 0.1, F)
    lo, hi = np.full(U, -1.0), np.full(U, 1.0)

    def step(refine):
        def leg():
            def fn():
                cem.optimize(state)
                if refine:
                    refine_plan(cem, state, cem.get_plan(), 3, 0.05, lo, hi)
            for _ in range(5):
                fn()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts))
        return leg
    cs = _alternate({"plain": step(False), "refined": step(True)}, rounds)
    lines += ["## CEM control step, N = 1000, 5 iterations, H = 30, plan readback on (Engine.optimize, wall clock)", "",
              "| step | time per control step [us] |", "|---|---|",
              "| optimize | %s |" % _fmt(cs["plain"]),
              "| optimize + get_plan + refine_plan(steps = 3): 4 gradient calls of one row, host in / host out | %s |" % _fmt(cs["refined"]),
              "| difference of the medians | %.1f |" % ((cs["refined"][0] - cs["plain"][0]) * 1e3), ""]

    if closed_loop:
        import plan_gradient_pendulum as X
        num_agents, task_horizon = 10, 200
        env = X.make_env(num_agents)
        handler, reward_model = X.learn(env, num_agents, task_horizon)
        lines += ["## Pendulum, learned 4-32-32-32-3 dynamics and 7-64-64-1 reward, CEM H = 30, 5 iterations, %d agents x %d steps" % (num_agents, task_horizon), "",
                  "| planner | mean closed-loop return | upright at the end |", "|---|---|---|"]
        for population in (50, 500):
            for steps in (0, 3):
                r, up = X.closed_loop_return(env, X.make_policy(handler, reward_model, num_agents, population, steps), task_horizon)
                lines.append("| CEM N = %d, refine_steps = %d | %.1f | %d / %d |" % (population, steps, r, up, num_agents))
        lines += ["", "Returns are negative costs (smaller magnitude is better); one seed, so differences of a few units are within what another seed would move.", ""]
    print("\n".join(lines))


if __name__ == "__main__":
    main(closed_loop="--no-closed-loop" not in sys.argv)
