#!/usr/bin/env python
"""What a user-supplied device function costs (run on a GPU box): Pendulum, CEM N=500 H=30 5 iterations (config 2's
size) with (a) the built-in fused kernel, (b) the built-in per-iteration kernels, (c) user reward + user dynamics in the
hiprtc-compiled fused rollout kernel, (d) the same through the step-wise evaluator.  us per control step.

--params (or after the above without it): runtime parameters (bbmpc_set_*_source_params) against the same numbers as
literals -- config-2-size user reward + user dynamics (fused and step-wise) with the goal and the mass as parameters,
HalfCheetah MLP + a goal reward (N=1000, H=30) -- and the old way of moving a goal, a new source string per goal: compile,
module load and one control step, end to end, against set_params + one control step."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rate(eng, start, steps=200):
    import torch
    dev = torch.device("cuda", 0)
    st = torch.from_numpy(start).to(dev)
    nx = torch.empty_like(st)
    rec = torch.zeros((start.shape[0], 5), device=dev)
    for _ in range(10):
        eng.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
        st, nx = nx, st
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
        st, nx = nx, st
    eng.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def params_section():
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.utils import synthetic as SY
    from test_gpu_user_params import ANGLE_REWARD, DYNAMICS_SIG, GOAL_REWARD, MASS_PENDULUM, REWARD_SIG, _forms
    out = {}
    goal, mass = [0.5, 0.001], [1.0]
    rp, rl = _forms(ANGLE_REWARD, REWARD_SIG, goal)
    dp, dl = _forms(MASS_PENDULUM, DYNAMICS_SIG, mass)
    kw = dict(dim_s=3, num_agents=1, planning_horizon=30, population_size=500, max_iterations=5, num_elite=50)
    start = SY.pendulum_start_states(1)

    def pend(par, env=None):
        if env:
            os.environ["BBMPC_USER_STEPWISE"] = env
        e = Engine(L.OPT_CEM, L.DYN_USER, L.REW_USER, [-2.0], [2.0], **kw)
        os.environ.pop("BBMPC_USER_STEPWISE", None)
        e.set_reward_source(rp if par else rl, 2 if par else 0)
        e.set_dynamics_source(dp if par else dl, 1 if par else 0)
        if par:
            e.set_user_params(L.USER_KIND_REWARD, goal)
            e.set_user_params(L.USER_KIND_DYNAMICS, mass)
        return e
    for form, env in (("fused", None), ("step-wise", "1")):
        out["config-2 size, user reward + user dynamics, %s: literals" % form] = rate(pend(False, env), start, 200)
        out["config-2 size, user reward + user dynamics, %s: parameters" % form] = rate(pend(True, env), start, 200)
    S, U = 20, 6
    ckw = dict(dim_s=S, num_agents=1, planning_horizon=30, population_size=1000, max_iterations=5, num_elite=50)
    cstart = SY.cheetah_start_states(1)
    cgoal = [0.5, 1.0, 0.001]
    crp, crl = _forms(GOAL_REWARD, REWARD_SIG, cgoal)
    for par in (False, True):
        e = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_USER, [-1.0] * U, [1.0] * U, **ckw)
        e.set_mlp(*SY.make_mlp_params(), [1, 1, 0], SY.cheetah_stats(S, U))
        e.set_reward_source(crp if par else crl, 3 if par else 0)
        if par:
            e.set_user_params(L.USER_KIND_REWARD, cgoal)
        out["HalfCheetah MLP + goal reward N=1000 H=30: %s" % ("parameters" if par else "literals")] = rate(e, cstart, 100)
    # moving the goal: a new literal source per goal (compile + module load + step) against set_params + step
    import torch
    dev = torch.device("cuda", 0)
    for form, env in (("fused", None), ("step-wise", "1")):
        lit, par = pend(False, env), pend(True, env)
        st = torch.from_numpy(start).to(dev)
        nx = torch.empty_like(st)
        rec = torch.zeros((1, 5), device=dev)
        for e in (lit, par):
            e.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
            e.synchronize()
        n_goals = 8
        t0 = time.perf_counter()
        for k in range(n_goals):
            lit.set_reward_source(_forms(ANGLE_REWARD, REWARD_SIG, [0.25 * (k + 1), 0.001])[1])
            lit.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
            lit.synchronize()
        out["goal change by new source string + step, %s" % form] = (time.perf_counter() - t0) / n_goals * 1e6
        c0 = par.compile_count()
        t0 = time.perf_counter()
        for k in range(n_goals):
            par.set_user_params(L.USER_KIND_REWARD, [0.25 * (k + 1), 0.001])
            par.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
            par.synchronize()
        out["goal change by set_user_params + step, %s" % form] = (time.perf_counter() - t0) / n_goals * 1e6
        assert par.compile_count() == c0
    return out


def main():
    if "--params" in sys.argv:
        from blackbox_mpc_amd import _build
        _build.build()
        for k, v in params_section().items():
            print("| %s | %.1f |" % (k, v))
        return
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.utils import synthetic as SY
    from test_gpu_user_functions import INTENDED_PENDULUM_REWARD, USER_PENDULUM_MODEL
    kw = dict(dim_s=3, num_agents=1, planning_horizon=30, population_size=500, max_iterations=5, num_elite=50)
    start = SY.pendulum_start_states(1)
    out = {}
    out["built-in, persistent kernel"] = rate(Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], **kw), start)
    os.environ["BBMPC_FUSED"] = "0"
    out["built-in, per-iteration kernels"] = rate(Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], **kw), start)
    del os.environ["BBMPC_FUSED"]
    for name, env in (("user reward + user dynamics, fused hiprtc rollout", None), ("user reward + user dynamics, step-wise", "1")):
        if env:
            os.environ["BBMPC_USER_STEPWISE"] = env
        e = Engine(L.OPT_CEM, L.DYN_USER, L.REW_USER, [-2.0], [2.0], **kw)
        os.environ.pop("BBMPC_USER_STEPWISE", None)
        e.set_reward_source(INTENDED_PENDULUM_REWARD)
        e.set_dynamics_source(USER_PENDULUM_MODEL)
        out[name] = rate(e, start, 100)
    # the common case: learned MLP dynamics + a custom reward (HalfCheetah MLP, CEM N=1000 H=30 5 iterations)
    from test_gpu_user_functions import USER_CHEETAH_REWARD
    S, U = 20, 6
    kw = dict(dim_s=S, num_agents=1, planning_horizon=30, population_size=1000, max_iterations=5, num_elite=50)
    cstart = SY.cheetah_start_states(1)

    def cheetah(rew, env=None):
        if env:
            os.environ["BBMPC_USER_STEPWISE"] = env
        e = Engine(L.OPT_CEM, L.DYN_MLP, rew, [-1.0] * U, [1.0] * U, **kw)
        os.environ.pop("BBMPC_USER_STEPWISE", None)
        e.set_mlp(*SY.make_mlp_params(), [1, 1, 0], SY.cheetah_stats(S, U))
        if rew == L.REW_USER:
            e.set_reward_source(USER_CHEETAH_REWARD)
        return e

    def rate27(eng, steps):
        import torch
        dev = torch.device("cuda", 0)
        st = torch.from_numpy(cstart).to(dev)
        nx = torch.empty_like(st)
        rec = torch.zeros((1, 27), device=dev)
        for _ in range(5):
            eng.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
            st, nx = nx, st
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.optimize_dev(st.data_ptr(), rec.data_ptr(), d_next_state=nx.data_ptr())
            st, nx = nx, st
        eng.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6
    out["MLP + built-in cheetah reward (4-particle MFMA kernel)"] = rate27(cheetah(L.REW_CHEETAH), 100)
    out["MLP + user reward: MFMA rollout records the trajectory, one scoring launch"] = rate27(cheetah(L.REW_USER), 100)
    out["MLP + user reward, step-wise"] = rate27(cheetah(L.REW_USER, "1"), 20)
    out.update(params_section())
    for k, v in out.items():
        print("| %s | %.1f |" % (k, v))


if __name__ == "__main__":
    main()
