"""What the learned policy prior (bbmpc_set_policy_prior_mlp, k_policy_prior_rollout) costs and what it buys.  Prints
markdown; the committed copy is profiles/policy_prior.md.

    python tools/policy_prior_rate.py > profiles/policy_prior.md

Method.  Every comparison alternates its legs (A B A B ...), `rounds` times; a leg is the median of `reps` timed calls
after a warm-up, and the table gives the median of the leg medians with their min .. max as the spread.
 * Kernels: bbmpc_predict_policy_rollouts_dev (k_policy_prior_rollout alone, both outputs wanted, sigma = 0.3 with a noise
   tensor of the caller's, so nothing else is launched) beside bbmpc_predict_trajectories_dev (k_traj_mlp alone, states
   wanted) at B = K rows, Hq = H = 30, the same 26-200-200-20 model; stream events on the handle's torch stream around one
   call.  k_traj_mlp compiles to what it compiled to in the parent commit (equal resource remarks).
 * Control steps: host-in / host-out Engine.optimize calls (wall clock), CEM, N = 1000, H = 30, 5 iterations, on the
   per-iteration route on both legs: plan readback is on (bbmpc_set_keep_plan), which routes the handle without the prior
   exactly as the parent commit routes it, and changes nothing for the handle with it.
 * Closed-loop return: examples/policy_prior_pendulum.py's setup, profiles/elite_carry.md's design -- the same start states
   for every leg, several optimizer seeds, paired differences (with - without) over (seed, agent) with their standard
   error."""
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


def main(reps=40, rounds=5, seeds=3):
    import torch
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    stream = torch.cuda.Stream()
    S, U, N, H = 20, 6, 1000, 30
    dyn, pol = [26, 200, 200, 20], [20, 200, 200, 6]
    acts = [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE]
    pw, pb = _params(pol, 2)
    lines = ["# Learned policy prior: measured cost and effect", "",
             "Produced by `tools/policy_prior_rate.py` on %s; its docstring states the method.  Times are medians over %d"
             % (torch.cuda.get_device_name(0), rounds),
             "alternating rounds of %d-call medians, spread = min .. max of the round medians." % reps, ""]

    def handle(**kw):
        eng = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_CHEETAH, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=1, planning_horizon=H,
                     population_size=N, max_iterations=5, num_elite=100, seed=1, **kw)
        ws, bs = _params(dyn, 1)
        ws[-1] *= F(0.05)
        eng.set_mlp(ws, bs, acts, None)
        return eng

    def timed(fn):
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

    # ---- the kernels ---------------------------------------------------------------------------------------------------------
    lines += ["## k_policy_prior_rollout beside k_traj_mlp, model 26-200-200-20, policy 20-200-200-6, H = 30, one agent", "",
              "`k_traj_mlp` is timed in THIS build, not in a build of the parent commit: the kernel was not edited and its resource",
              "remarks equal the parent's (DESIGN.md section 8l), so it is the parent's kernel.", "",
              "| rows | k_traj_mlp (this build = the parent's kernel), B = K [us] | k_policy_prior_rollout, K [us] | ratio |", "|---|---|---|---|"]
    for K in (16, 64):
        eng = handle()
        eng.set_policy_prior_mlp(pw, pb, acts, None, count=K, noise_std=0.3)
        eng.set_torch_stream(stream)
        st1 = torch.zeros((1, S), device="cuda") + 0.1
        stK = torch.zeros((K, S), device="cuda") + 0.1
        seq = (torch.rand((K, H, U), device="cuda") * 2 - 1).contiguous()
        xi = torch.randn((1, K, H, U), device="cuda").contiguous()
        so = torch.empty((K, H, S), device="cuda")
        ao = torch.empty((K, 1, H, U), device="cuda")
        so2 = torch.empty((K, 1, H, S), device="cuda")
        torch.cuda.synchronize()
        legs = {"traj": lambda: timed(lambda: eng.predict_trajectories_dev(stK.data_ptr(), seq.data_ptr(), K, H, so.data_ptr(), 0)),
                "prior": lambda: timed(lambda: eng.predict_policy_rollouts_dev(st1.data_ptr(), xi.data_ptr(), ao.data_ptr(), so2.data_ptr()))}
        r = _alternate(legs, rounds)
        lines.append("| %d | %s | %s | %.2f |" % (K, _fmt(r["traj"]), _fmt(r["prior"]), r["prior"][0] / r["traj"][0]))
    lines.append("")

    # ---- control steps ---------------------------------------------------------------------------------------------------------
    def step_leg(eng_, state):
        def leg():
            for _ in range(10):
                eng_.optimize(state)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                eng_.optimize(state)
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts))
        return leg
    state = np.full((1, S), 0.1, F)
    e0, e16, e64 = handle(), handle(), handle()
    for e in (e0, e16, e64):
        e.set_keep_plan(True)
    e16.set_policy_prior_mlp(pw, pb, acts, None, count=16, noise_std=0.3)
    e64.set_policy_prior_mlp(pw, pb, acts, None, count=64, noise_std=0.3)
    cs = _alternate({"0": step_leg(e0, state), "16": step_leg(e16, state), "64": step_leg(e64, state)}, rounds)
    lines += ["## Control step, CEM, 5 iterations, N = 1000, H = 30, 26-200-200-20 + built-in cheetah reward (Engine.optimize, wall clock, per-iteration route)", "",
              "| handle | time per control step [us] |", "|---|---|",
              "| no prior (the parent commit's per-iteration route) | %s |" % _fmt(cs["0"]),
              "| prior, K = 16 (+ draw into the buffer, k_gen_policy_noise, k_policy_prior_rollout per iteration) | %s |" % _fmt(cs["16"]),
              "| prior, K = 64 | %s |" % _fmt(cs["64"]), "",
              "The prior adds %.1f us (K = 16) and %.1f us (K = 64) per control step, %.1f and %.1f us per iteration."
              % ((cs["16"][0] - cs["0"][0]) * 1e3, (cs["64"][0] - cs["0"][0]) * 1e3, (cs["16"][0] - cs["0"][0]) * 200, (cs["64"][0] - cs["0"][0]) * 200), ""]

    # ---- closed-loop return on the pendulum ----------------------------------------------------------------------------------
    import policy_prior_pendulum as X
    num_agents, task_horizon = 10, 200
    env = X.make_env(num_agents)
    handler, value, prior = X.learn(env, num_agents, task_horizon)

    def returns(population, net, seed):
        polc = X.make_policy(handler, num_agents, 10, population, value, net, 8 if net is not None else 0, 0.3, seed=seed)
        from blackbox_mpc_amd.utils.rollouts import perform_rollouts
        _, _, rews = perform_rollouts(env, 1, task_horizon, polc)
        return np.sum(rews[0], axis=0).reshape(-1).astype(np.float64)                  # per agent
    lines += ["## Pendulum, learned 4-32-32-32-3 dynamics, H = 10 + V, policy 3-64-64-1 cloned from a (H = 30, N = 500) controller; %d agents x %d steps x %d seeds" % (num_agents, task_horizon, seeds), "",
              "| population | mean return, no prior | mean return, 8 policy rollouts (sigma 0.3) | paired difference (with - without) +- standard error |", "|---|---|---|---|"]
    for population in (500, 200, 100, 50):
        a = np.concatenate([returns(population, None, s) for s in range(seeds)])
        b = np.concatenate([returns(population, prior, s) for s in range(seeds)])
        d = b - a
        lines.append("| %d | %.1f | %.1f | %+.1f +- %.1f |" % (population, a.mean(), b.mean(), d.mean(), d.std(ddof=1) / np.sqrt(d.size)))
    lines += ["", "(Returns are negative costs: a positive difference means the prior helped.)", ""]
    print("\n".join(lines))


if __name__ == "__main__":
    main()
