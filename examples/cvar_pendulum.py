"""Risk-sensitive planning through the learned model of examples/learn_dynamics_and_control.py: the same tutorial, then a
ParticleTrajectoryEvaluator with risk_alpha = 0.2 -- every candidate is rolled out 20 times with the model's measured
one-step residual as process noise and scored by the mean of its 4 worst returns (CVaR) -- and the 5 % / 95 % band of the
states the plan is predicted to visit.

    python examples/cvar_pendulum.py
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
from blackbox_mpc_amd.utils.iterative_mpc import learn_dynamics_iteratively_w_mpc    # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402
from blackbox_mpc_amd.utils.rollouts import ModelEnvironment                         # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
num_agents, task_horizon, planning_horizon = 4, 100, 20

rng = np.random.default_rng(0)
theta0 = rng.uniform(-np.pi, np.pi, num_agents)
start = np.stack([np.cos(theta0), np.sin(theta0), rng.uniform(-1, 1, num_agents)], axis=1).astype(np.float32)
true_handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)

handler, _ = learn_dynamics_iteratively_w_mpc(
    env, number_of_initial_rollouts=5, number_of_rollouts_for_refinement=1, number_of_refinement_steps=1,
    task_horizon=task_horizon, env_action_space=action_space, env_observation_space=observation_space,
    initial_policy=RandomPolicy(num_agents, action_space, seed=0), planning_horizon=planning_horizon,
    reward_function=pendulum_reward_function, optimizer_name="CEM", num_agents=num_agents,
    dynamics_function=DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=0),
    epochs=20, learning_rate=1e-3, batch_size=128, train_args={"seed": 0}, population_size=200, num_elite=20, max_iterations=3)
sigma = handler.residual_std()
print("one-step residual of the learned model (the process noise):", sigma)

evaluator = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=20, process_noise_std=sigma, risk_alpha=0.2)
print("scoring rule (kind, tail_count):", evaluator.risk_settings)
policy = MPCPolicy(trajectory_evaluator=evaluator, env_action_space=action_space, env_observation_space=observation_space,
                   optimizer_name="CEM", num_agents=num_agents, planning_horizon=planning_horizon, population_size=200, num_elite=20,
                   max_iterations=3, seed=0)
policy.keep_plan(True)
action, _, _ = policy.act(start, 0)
actions, state_mean, state_std, reward_mean, reward_std, state_q, reward_q = policy.plan_distribution(start, quantiles=[0.05, 0.95])
print("first action per agent:", action[:, 0])
print("agent 0, angular velocity along the plan:  step   5 %     mean    95 %")
for t in range(0, planning_horizon, 4):
    print("                                           %3d  %7.3f %7.3f %7.3f" % (t, state_q[0, 0, t, 2], state_mean[0, t, 2], state_q[0, 1, t, 2]))
print("agent 0, predicted plan return: 5 %% step rewards sum to %.1f, mean %.1f, 95 %% %.1f"
      % (reward_q[0, 0].sum(), reward_mean[0].sum(), reward_q[0, 1].sum()))
