"""Gradient steps inside CEM (GradCEM, Bharadhwaj et al. 2020): a DeterministicMLP learns the pendulum's dynamics and a
LearnedRewardMLP its reward from random-policy episodes (examples/plan_gradient_pendulum.py's setup); CEM plans through both
networks and, with grad_steps > 0, every iteration moves its candidates by that many Adam steps on the model return before
the elites are chosen (Engine.set_grad_refine: gather, k_plan_grad + step kernel, scatter, all on the device).  The
closed-loop return on the real system is printed for plain CEM, for CEM followed by three refinement steps on its plan
(on the device: refine_device=True) and for GradCEM, at a small and a larger population.

    python examples/gradcem_pendulum.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_gradient_pendulum as base                                                # noqa: E402
from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy                           # noqa: E402
from blackbox_mpc_amd.utils.rollouts import perform_rollouts                         # noqa: E402


def make_policy(handler, reward_model, num_agents, population, **kw):
    return MPCPolicy(reward_function=reward_model, env_action_space=base.action_space, env_observation_space=base.observation_space,
                     dynamics_handler=handler, optimizer_name="CEM", num_agents=num_agents, planning_horizon=30,
                     population_size=population, num_elite=max(4, population // 10), max_iterations=5, **kw)


PLANNERS = [("plain CEM", dict()),
            ("CEM + refine_steps=3 on the device", dict(refine_steps=3, refine_lr=0.05, refine_device=True)),
            ("GradCEM, grad_steps=1", dict(grad_steps=1, grad_lr=0.05)),
            ("GradCEM, grad_steps=3", dict(grad_steps=3, grad_lr=0.05))]


def episode_returns(env, policy, task_horizon):
    """per-agent closed-loop returns [A] (every agent is an episode from its own start state)"""
    _, _, rews = perform_rollouts(env, 1, task_horizon, policy)
    return np.sum(np.asarray(rews[0], np.float64), axis=0)


if __name__ == "__main__":
    num_agents, task_horizon = 10, 200
    env = base.make_env(num_agents)
    handler, reward_model = base.learn(env, num_agents, task_horizon)
    for population in (50, 500):
        for name, kw in PLANNERS:
            r = episode_returns(env, make_policy(handler, reward_model, num_agents, population, **kw), task_horizon)
            print("N = %3d, %-36s mean closed-loop return %8.1f +- %.1f (standard error over %d episodes)"
                  % (population, name + ":", r.mean(), r.std(ddof=1) / np.sqrt(len(r)), len(r)))
