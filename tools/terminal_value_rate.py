"""What a learned terminal value (bbmpc_set_terminal_value_mlp, k_value_mlp_terminal) costs and what it buys.  Prints
markdown; the committed copy is profiles/terminal_value.md.

    python tools/terminal_value_rate.py > profiles/terminal_value.md

Method.  Every comparison alternates its legs (A B A B ...), `rounds` times; a leg is the median of `reps` timed calls
after a warm-up, and the table gives the median of the leg medians with their min .. max as the spread.
 * k_value_mlp_terminal has no profiling bracket of its own.  It is timed as the difference of one evaluate_dev (stream
   events on the handle's torch stream) on a BBMPC_REW_MLP handle with the value network installed and removed: that
   handle's route is the same in both legs (trajectory recorded either way), so the difference is the one extra launch,
   kernel plus launch gap.
 * Control steps are host-in / host-out Engine.optimize calls (wall clock), the form MPCPolicy.act uses and the one the
   parent's hipGraph replay serves: PI2, N = 1000, 5 iterations, 26-200-200-20 model, built-in cheetah reward.
 * Closed-loop returns: examples/terminal_value_pendulum.py's setup, the same start states for every leg."""
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
    """legs: {label: callable -> one leg's median in ms}; -> {label: (median of medians, min, max)}"""
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(fn())
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in got.items()}


def _fmt(t):
    return "%.1f (%.1f .. %.1f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)


def main(reps=40, rounds=5):
    import torch
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    stream = torch.cuda.Stream()
    S, U, N = 20, 6, 1000
    dyn, val = [26, 200, 200, 20], [20, 200, 200, 1]
    acts = [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE]
    vw, vb = _params(val, 2)
    lines = ["# Learned terminal value: measured cost and effect", "",
             "Produced by `tools/terminal_value_rate.py` on %s; its docstring states the method.  Times are medians over %d"
             % (torch.cuda.get_device_name(0), rounds),
             "alternating rounds of %d-call medians, spread = min .. max of the round medians." % reps, ""]

    def handle(H, reward, opt=L.OPT_NONE, **kw):
        eng = Engine(opt, L.DYN_MLP, reward, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=1, planning_horizon=H, **kw)
        ws, bs = _params(dyn, 1)
        ws[-1] *= F(0.05)
        eng.set_mlp(ws, bs, acts, None)
        return eng

    # ---- the kernel: one extra launch behind an unchanged route ------------------------------------------------------------
    H = 30
    eng = handle(H, L.REW_MLP)
    rw, rb = _params([46, 200, 200, 1], 3)
    eng.set_reward_mlp(rw, rb, acts, 7, None)
    eng.set_torch_stream(stream)
    st = torch.zeros((1, S), device="cuda") + 0.1
    seq = (torch.rand((N, 1, H, U), device="cuda") * 2 - 1).contiguous()
    out = torch.empty((N, 1), device="cuda")
    torch.cuda.synchronize()

    def evaluate_leg(with_value):
        def leg():
            if with_value:
                eng.set_terminal_value_mlp(vw, vb, acts, None, 1.0)
            else:
                eng.set_terminal_value_mlp(None, None, None)
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
    ev = _alternate({"without": evaluate_leg(False), "with": evaluate_leg(True)}, rounds)
    lines += ["## k_value_mlp_terminal, value network 20-200-200-1, N = 1000 (63 workgroups of 13 waves)", "",
              "| evaluate_dev on a REW_MLP handle, H = 30 | time [us] |", "|---|---|",
              "| value network removed | %s |" % _fmt(ev["without"]),
              "| value network installed | %s |" % _fmt(ev["with"]),
              "| difference of the medians: the one extra launch (kernel + launch gap) | %.1f |" % ((ev["with"][0] - ev["without"][0]) * 1e3), ""]

    # ---- control steps: host-in / host-out, PI2, built-in cheetah reward -----------------------------------------------------
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
    e30, e30v, e10, e10v = handle(30, L.REW_CHEETAH, **kw), handle(30, L.REW_CHEETAH, **kw), handle(10, L.REW_CHEETAH, **kw), handle(10, L.REW_CHEETAH, **kw)
    e30v.set_terminal_value_mlp(vw, vb, acts, None, 1.0)
    e10v.set_terminal_value_mlp(vw, vb, acts, None, 1.0)
    cs = _alternate({"H30": step_leg(e30, state), "H30V": step_leg(e30v, state), "H10": step_leg(e10, state), "H10V": step_leg(e10v, state)}, rounds)
    replayed = e30.graph_stats() if hasattr(e30, "graph_stats") else None
    ratio = cs["H10V"][0] / cs["H30"][0]
    faster = cs["H10V"][2] < cs["H30"][1]
    lines += ["## Control step, PI2, 5 iterations, N = 1000, 26-200-200-20 + built-in cheetah reward (Engine.optimize, wall clock)", "",
              "| handle | time per control step [us] |", "|---|---|",
              "| H = 30, no value network (this build's graph-replayed step%s) | %s |" % ("" if replayed is None else "; replays counted: %s" % (replayed,), _fmt(cs["H30"])),
              "| H = 30, value network (per-launch path, trajectory recorded, + k_value_mlp_terminal per iteration) | %s |" % _fmt(cs["H30V"]),
              "| H = 10, no value network | %s |" % _fmt(cs["H10"]),
              "| H = 10, value network | %s |" % _fmt(cs["H10V"]), "",
              "Leaving the graph and recording at H = 30 costs %.1f us per control step (%.2f x)." % ((cs["H30V"][0] - cs["H30"][0]) * 1e3, cs["H30V"][0] / cs["H30"][0]),
              "(H = 10, V) against (H = 30, no V): %.2f x the time.  %s" % (ratio,
               "The slowest H = 10 + V round is faster than the fastest H = 30 round: faster by more than the run-to-run spread." if faster else
               "The spreads overlap or the short-horizon step is slower: NOT faster than the H = 30 step by more than the run-to-run spread."), ""]

    # ---- closed-loop return on the pendulum ----------------------------------------------------------------------------------
    import terminal_value_pendulum as X
    num_agents, task_horizon = 10, 200
    env = X.make_env(num_agents)
    handler, value = X.learn(env, num_agents, task_horizon)
    lines += ["## Pendulum, learned 4-32-32-32-3 dynamics, V = 3-64-64-1 on %d-step returns (gamma %.2f), CEM N = 500, %d agents x %d steps" % (X.N_STEP, X.GAMMA, num_agents, task_horizon), "",
              "| planner | mean closed-loop return | upright at the end |", "|---|---|---|"]
    rets = {}
    for label, horizon, v in (("H = 30, no V", 30, None), ("H = 10, no V", 10, None), ("H = 10, V", 10, value)):
        rets[label], up = X.closed_loop_return(env, X.make_policy(handler, num_agents, horizon, v), task_horizon)
        lines.append("| %s | %.1f | %d / %d |" % (label, rets[label], up, num_agents))
    lines += ["", "(H = 10, V) against (H = 30, no V): return %.1f against %.1f (ratio %.2f; returns are negative costs, smaller magnitude is better)."
              % (rets["H = 10, V"], rets["H = 30, no V"], rets["H = 10, V"] / rets["H = 30, no V"]), ""]
    print("\n".join(lines))


if __name__ == "__main__":
    main()
