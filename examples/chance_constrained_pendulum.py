"""Chance-constrained planning through the learned model of examples/learn_dynamics_and_control.py: the same tutorial, then
a ParticleTrajectoryEvaluator with the model's measured one-step residual as process noise, run closed loop on the true
pendulum twice -- without and with a StateBoxConstraint that limits |angular velocity| -- and for each the share of real
steps outside the limit and the return.

    python examples/chance_constrained_pendulum.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP   # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies import MPCPolicy, RandomPolicy                        # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator, ParticleTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.constraints import StateBoxConstraint                    # noqa: E402
from blackbox_mpc_amd.utils.iterative_mpc import learn_dynamics_iteratively_w_mpc    # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402
from blackbox_mpc_amd.utils.rollouts import ModelEnvironment                         # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
num_agents, task_horizon, planning_horizon = 4, 100, 20
SPEED_LIMIT = 4.0

rng = np.random.default_rng(0)
theta0 = rng.uniform(-np.pi, np.pi, num_agents)
start = np.stack([np.cos(theta0), np.sin(theta0), rng.uniform(-1, 1, num_agents)], axis=1).astype(np.float32)
true_handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
true_evaluator = DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler)
env = ModelEnvironment(true_evaluator, start)

handler, _ = learn_dynamics_iteratively_w_mpc(
    env, number_of_initial_rollouts=5, number_of_rollouts_for_refinement=1, number_of_refinement_steps=1,
    task_horizon=task_horizon, env_action_space=action_space, env_observation_space=observation_space,
    initial_policy=RandomPolicy(num_agents, action_space, seed=0), planning_horizon=planning_horizon,
    reward_function=pendulum_reward_function, optimizer_name="CEM", num_agents=num_agents,
    dynamics_function=DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=0),
    epochs=20, learning_rate=1e-3, batch_size=128, train_args={"seed": 0}, population_size=200, num_elite=20, max_iterations=3)
sigma = handler.residual_std()
print("one-step residual of the learned model (the process noise):", sigma)

box = StateBoxConstraint(low=[-np.inf, -np.inf, -SPEED_LIMIT], high=[np.inf, np.inf, SPEED_LIMIT], max_violation=0.05, weight=1e3)
for constraint in (None, box):
    evaluator = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=20, process_noise_std=sigma, constraint=constraint)
    policy = MPCPolicy(trajectory_evaluator=evaluator, constraint=constraint, env_action_space=action_space,
                       env_observation_space=observation_space, optimizer_name="CEM", num_agents=num_agents,
                       planning_horizon=planning_horizon, population_size=200, num_elite=20, max_iterations=3, seed=0)
    policy.keep_plan(constraint is not None)
    state, total, outside, planned = start.copy(), np.zeros(num_agents), 0, []
    for t in range(task_horizon):
        action, _, _ = policy.act(state, t)
        if constraint is not None and t % 20 == 0:
            planned.append(policy.plan_violation(state))
        nxt = true_evaluator.predict_next_state(state, action)
        total += true_evaluator.evaluate_next_reward(state, nxt, action)
        outside += int(np.sum(np.abs(nxt[:, 2]) > SPEED_LIMIT))
        state = nxt
    print("%s: share of real steps with |angular velocity| > %.1f: %.3f, mean return %.1f"
          % ("with the constraint" if constraint is not None else "without a constraint", SPEED_LIMIT,
             outside / (task_horizon * num_agents), total.mean()))
    if planned:
        print("  violation probability of the plan at steps 0, 20, ..: %s" % np.round(np.mean(planned, axis=1), 3))
