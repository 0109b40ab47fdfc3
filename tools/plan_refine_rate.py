"""What plan refinement on the device (bbmpc_refine_plans) and gradient steps inside CEM (bbmpc_set_grad_refine) cost and buy.
Prints markdown; the committed copy is profiles/plan_refine.md.

    python tools/plan_refine_rate.py > profiles/plan_refine.md

Method.  Every comparison alternates its legs (A B A B ...), `rounds` times; a leg is the median of `reps` timed calls after
a warm-up, and the tables give the median of the leg medians with their min .. max as the spread.  Wall clock, host arrays
in and out, unless a row says otherwise.  Networks as in profiles/plan_gradient.md: 26-200-200-20 dynamics, 46-200-200-1
reward, 20-200-200-1 value.
 * Refinement: three steps with keep-best (four gradient calls), Hq = 30, B = 1 and B = 1000.  The host leg is
   utils.plan_refinement.refine_plan on Engine.plan_gradient -- the path the handle had before; the device leg is
   Engine.refine_plans.  A third row times refine_plans_dev on device arrays with stream events.
 * Control step: Engine.optimize of a CEM handle (N = 1000, 5 iterations, H = 30) with grad_steps 0, 1 and 3 on all
   candidates, beside one plan_gradient_dev call of 1000 rows (stream events).
 * Closed loop: examples/gradcem_pendulum.py's planners on the pendulum with learned dynamics and reward, the same start
   states for every leg; mean and standard error over the agents' episodes."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from plan_gradient_rate import _alternate, _fmt, _params        # noqa: E402
F = np.float32


def main(reps=20, rounds=5, closed_loop=True):
    import torch
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan
    stream = torch.cuda.Stream()
    S, U, H = 20, 6, 30
    acts = [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE]
    lines = ["# Plan refinement on the device and gradient steps inside CEM: measured cost and effect", "",
             "Produced by `tools/plan_refine_rate.py` on %s; its docstring states the method.  Times are medians over %d"
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

    def wall(fn):
        def leg():
            for _ in range(3):
                fn()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts))
        return leg

    def events(fn):
        def leg():
            for _ in range(3):
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

    eng = handle()
    eng.set_torch_stream(stream)
    lo, hi = np.full(U, -1.0), np.full(U, 1.0)
    rng = np.random.default_rng(0)
    lines += ["## Three refinement steps with keep-best (four gradient calls), Hq = 30", "",
              "| B | host loop: refine_plan on plan_gradient [us] | device: refine_plans [us] | host / device | refine_plans_dev, device arrays, stream events [us] |",
              "|---|---|---|---|---|"]
    for B in (1, 1000):
        st = (rng.random((B, S)) - 0.5).astype(F)
        seq = (rng.random((B, H, U)) * 2 - 1).astype(F)
        d_st, d_seq, d_work, d_ret = torch.tensor(st, device="cuda"), torch.tensor(seq, device="cuda"), torch.empty((B, H, U), device="cuda"), torch.empty((B,), device="cuda")
        torch.cuda.synchronize()

        def dev_call():
            with torch.cuda.stream(stream):
                d_work.copy_(d_seq)
            eng.refine_plans_dev(d_st.data_ptr(), d_work.data_ptr(), B, H, 3, 0.05, "adam", True, d_ret.data_ptr())
        r = _alternate({"host": wall(lambda: refine_plan(eng, st, seq, 3, 0.05, lo, hi)),
                        "device": wall(lambda: eng.refine_plans(st, seq, 3, 0.05)),
                        "dev": events(dev_call)}, rounds)
        print("refinement B = %d done" % B, file=sys.stderr, flush=True)
        lines.append("| %d | %s | %s | %.2f | %s |" % (B, _fmt(r["host"]), _fmt(r["device"]), r["host"][0] / r["device"][0], _fmt(r["dev"])))
    lines.append("")

    # ---- control step with gradient steps on all candidates --------------------------------------------------------------------
    N, iters = 1000, 5
    state = np.full((1, S), 0.1, F)
    cems = {}
    for g in (0, 1, 3):
        cems[g] = handle(opt=L.OPT_CEM, population_size=N, max_iterations=iters, num_elite=100, seed=1)
        if g:
            cems[g].set_grad_refine(g, 0.05, "adam", 0)
    st = (torch.rand((N, S), device="cuda") - 0.5).contiguous()
    seq = (torch.rand((N, H, U), device="cuda") * 2 - 1).contiguous()
    ret, grad = torch.empty((N,), device="cuda"), torch.empty((N, H, U), device="cuda")
    torch.cuda.synchronize()
    legs = {("cem", g): wall(lambda e=e: e.optimize(state)) for g, e in cems.items()}
    legs["grad"] = events(lambda: eng.plan_gradient_dev(st.data_ptr(), seq.data_ptr(), N, H, ret.data_ptr(), grad.data_ptr()))
    cs = _alternate(legs, rounds)
    print("control step done", file=sys.stderr, flush=True)
    lines += ["## CEM control step, N = 1000, 5 iterations, H = 30, gradient steps on all candidates (Engine.optimize, wall clock)", "",
              "| grad_steps | time per control step [us] | added per iteration [us] | added per iteration and gradient step [us] |", "|---|---|---|---|",
              "| 0 | %s | | |" % _fmt(cs[("cem", 0)])]
    for g in (1, 3):
        add = (cs[("cem", g)][0] - cs[("cem", 0)][0]) * 1e3 / iters
        lines.append("| %d | %s | %.1f | %.1f |" % (g, _fmt(cs[("cem", g)]), add, add / g))
    lines += ["| one plan_gradient_dev call, B = 1000, Hq = 30 (stream events) | %s | | |" % _fmt(cs["grad"]), ""]

    if closed_loop:
        import gradcem_pendulum as X
        num_agents, task_horizon = 10, 200
        env = X.base.make_env(num_agents)
        handler, reward_model = X.base.learn(env, num_agents, task_horizon)
        lines += ["## Pendulum, learned 4-32-32-32-3 dynamics and 7-64-64-1 reward, CEM H = 30, 5 iterations, %d episodes x %d steps" % (num_agents, task_horizon), "",
                  "| N | planner | mean closed-loop return | standard error |", "|---|---|---|---|"]
        for population in (50, 100, 500):
            for name, kw in X.PLANNERS:
                if "refine_steps" in kw:
                    kw = dict(kw, refine_device=False)           # the post-hoc polish as the handle had it: the host loop
                    name = "CEM + refine_steps=3 (host loop)"
                r = X.episode_returns(env, X.make_policy(handler, reward_model, num_agents, population, **kw), task_horizon)
                print("closed loop N = %d, %s done" % (population, name), file=sys.stderr, flush=True)
                lines.append("| %d | %s | %.1f | %.1f |" % (population, name, r.mean(), r.std(ddof=1) / np.sqrt(len(r))))
        lines += ["", "Returns are negative costs (smaller magnitude is better); one training seed.", ""]
    print("\n".join(lines))


if __name__ == "__main__":
    main(closed_loop="--no-closed-loop" not in sys.argv)
