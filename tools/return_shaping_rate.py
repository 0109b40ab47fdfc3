"""What discounted, termination-aware returns (bbmpc_set_return_shaping, k_shaped_return) cost.  Prints markdown; the
committed copy is profiles/return_shaping.md.

    python tools/return_shaping_rate.py > profiles/return_shaping.md

Method (that of tools/terminal_value_rate.py).  Every comparison alternates its legs (A B A B ...), `rounds` times; a leg is
the median of `reps` timed calls after a warm-up, and the table gives the median of the leg medians with min .. max as the
spread.
 * The shaped path per rollout: one evaluate_dev (stream events on the handle's torch stream), shaping on against off, on
   the same handle -- for the built-in cheetah reward (off: the in-kernel reward, nothing recorded) and for BBMPC_REW_MLP
   with a value network (off: k_reward_mlp_finish + k_value_mlp_terminal; on: k_reward_mlp_rows + k_shaped_return).
 * Control steps are host-in / host-out Engine.optimize calls (wall clock): PI2, N = 1000, H = 30, 5 iterations,
   26-200-200-20 model.  Without shaping the built-in-reward handle takes the graph-replayed step.
 * The example's violation shares and returns: examples/termination_pendulum.py's setup."""
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


def main(reps=40, rounds=5, example=True):
    import torch
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    stream = torch.cuda.Stream()
    S, U, N, H = 20, 6, 1000, 30
    acts = [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE]
    vw, vb = _params([20, 200, 200, 1], 2)
    rw, rb = _params([46, 200, 200, 1], 3)
    lo, hi = np.full(S, -np.inf, F), np.full(S, np.inf, F)
    hi[0] = 0.3                                               # a bound that part of the candidates cross
    lines = ["# Discounted, termination-aware returns: measured cost", "",
             "Produced by `tools/return_shaping_rate.py` on %s; its docstring states the method.  Times are medians over %d"
             % (torch.cuda.get_device_name(0), rounds),
             "alternating rounds of %d-call medians, spread = min .. max of the round medians." % reps, ""]

    def handle(reward, value, opt=L.OPT_NONE, **kw):
        eng = Engine(opt, L.DYN_MLP, reward, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=1, planning_horizon=H, **kw)
        ws, bs = _params([26, 200, 200, 20], 1)
        ws[-1] *= F(0.05)
        eng.set_mlp(ws, bs, acts, None)
        if reward == L.REW_MLP:
            eng.set_reward_mlp(rw, rb, acts, 7, None)
        if value:
            eng.set_terminal_value_mlp(vw, vb, acts, None, 1.0)
        return eng

    def shape(eng, on):
        if on:
            eng.set_return_shaping(0.99, lo, hi, -5.0)
        else:
            eng.set_return_shaping(1.0)

    # ---- per rollout: evaluate_dev, shaping on against off on one handle ---------------------------------------------------
    st = torch.zeros((1, S), device="cuda") + 0.1
    seq = (torch.rand((N, 1, H, U), device="cuda") * 2 - 1).contiguous()
    out = torch.empty((N, 1), device="cuda")
    torch.cuda.synchronize()

    def evaluate_leg(eng, on):
        def leg():
            shape(eng, on)
            fn = lambda: eng.evaluate_dev(st.data_ptr(), seq.data_ptr(), N, out.data_ptr())
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
    lines += ["## One rollout of N = 1000 candidates, H = 30, 26-200-200-20 (evaluate_dev, stream events)", "",
              "| handle | shaping off [us] | shaping on [us] | difference of the medians [us] |", "|---|---|---|---|"]
    for label, reward, value in (("built-in cheetah reward", L.REW_CHEETAH, False), ("BBMPC_REW_MLP 46-200-200-1 + V 20-200-200-1", L.REW_MLP, True)):
        eng = handle(reward, value)
        eng.set_torch_stream(stream)
        ev = _alternate({"off": evaluate_leg(eng, False), "on": evaluate_leg(eng, True)}, rounds)
        lines.append("| %s | %s | %s | %.1f |" % (label, _fmt(ev["off"]), _fmt(ev["on"]), (ev["on"][0] - ev["off"][0]) * 1e3))
    lines.append("")

    # ---- control steps: host-in / host-out, PI2 ------------------------------------------------------------------------------
    def step_leg(eng_, state):
        def leg():
            for _ in range(10):                                # (the graph is captured from the fifth identical call on)
                eng_.optimize(state)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                eng_.optimize(state)
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts))
        return leg
    state = np.full((1, S), 0.1, F)
    kw = dict(opt=L.OPT_PI2, population_size=N, max_iterations=5, seed=1)
    lines += ["## Control step, PI2, 5 iterations, N = 1000, H = 30 (Engine.optimize, wall clock)", "",
              "| handle | undiscounted path [us] | shaped path [us] | ratio |", "|---|---|---|---|"]
    for label, reward, value in (("built-in cheetah reward (off: the graph-replayed step)", L.REW_CHEETAH, False),
                                 ("BBMPC_REW_MLP + V (off: per launch, recorded)", L.REW_MLP, True)):
        plain, shaped = handle(reward, value, **kw), handle(reward, value, **kw)
        shape(shaped, True)
        cs = _alternate({"off": step_leg(plain, state), "on": step_leg(shaped, state)}, rounds)
        lines.append("| %s | %s | %s | %.2f |" % (label, _fmt(cs["off"]), _fmt(cs["on"]), cs["on"][0] / cs["off"][0]))
        if reward == L.REW_MLP:
            inside = cs["on"][0] <= cs["off"][2]
            lines += ["", "BBMPC_REW_MLP + V: the shaped step's median is %s the unshaped step's spread." % ("within" if inside else "ABOVE")]
    lines.append("")

    # ---- the example ---------------------------------------------------------------------------------------------------------
    if example:
        import termination_pendulum as X
        num_agents, task_horizon = 10, 200
        env, box = X.make_env(num_agents), X.speed_box()
        handler, value = X.learn(env, num_agents, task_horizon, box)
        lines += ["## Pendulum with a speed limit |thdot| <= %.0f, learned 4-32-32-32-3 dynamics, V = 3-64-64-1, discount %.2f, CEM N = 500, H = %d, %d agents x %d steps"
                  % (X.SPEED_LIMIT, X.GAMMA, X.HORIZON, num_agents, task_horizon), "",
                  "| planner | executed steps outside the box | mean return |", "|---|---|---|"]
        for label, b in (("no termination", None), ("termination, c = %.0f" % X.TERMINAL_REWARD, box)):
            share, ret = X.violation_share_and_return(env, X.make_policy(handler, num_agents, value, b), task_horizon, box)
            lines.append("| %s | %.1f %% | %.1f |" % (label, 100 * share, ret))
        lines.append("")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
