"""Train an MLP dynamics model on random rollouts of the pendulum and print how its open-loop error grows with the
number of steps it is rolled without correction -- the planner uses it for 30 steps at a time, the training loss only
sees one.

    python examples/multistep_model_error.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP   # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies import RandomPolicy                                   # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.dynamics_learning import learn_dynamics_from_policy      # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402
from blackbox_mpc_amd.utils.rollouts import ModelEnvironment, perform_rollouts       # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
num_agents, task_horizon = 10, 200

rng = np.random.default_rng(0)
theta0 = rng.uniform(-np.pi, np.pi, num_agents)
start = np.stack([np.cos(theta0), np.sin(theta0), rng.uniform(-1, 1, num_agents)], axis=1).astype(np.float32)
true_handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)
policy = RandomPolicy(num_agents, action_space, seed=0)

handler = learn_dynamics_from_policy(
    env, policy, number_of_rollouts=5, task_horizon=task_horizon,
    dynamics_function=DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=0),
    epochs=30, learning_rate=1e-3, batch_size=128, seed=0, multistep_horizon=30)
rmse, windows = handler.multistep_rmse
print("one-step validation loss %.5f; open-loop rmse over %d windows of the training episodes:" % (handler.validation_loss[-1], windows))
for k in (1, 10, 30):
    print("  %2d-step error  cos %.4f  sin %.4f  thdot %.4f" % (k, rmse[k - 1, 0], rmse[k - 1, 1], rmse[k - 1, 2]))

# the same on fresh episodes the model has not seen, and for the true model on its own data (~0)
obs, acs, _ = perform_rollouts(env, 2, task_horizon, policy)
fresh, n = handler.multistep_error(obs, acs, 30)
print("fresh episodes (%d windows): 1 / 10 / 30-step thdot rmse %.4f / %.4f / %.4f" % (n, fresh[0, 2], fresh[9, 2], fresh[29, 2]))
print("true model on its own episodes: max rmse %.2e" % true_handler.multistep_error(obs, acs, 30)[0].max())
