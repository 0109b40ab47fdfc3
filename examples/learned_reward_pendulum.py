"""Plan with a reward that was never written down: the environment only RETURNS reward samples.  A DeterministicMLP
learns the pendulum's dynamics and a LearnedRewardMLP its reward r(s, a, s') from the same random-policy episodes; CEM
then controls the real system through both networks (the reward network runs on the matrix cores over the states the
model rollouts produce).  The closed-loop return is printed beside the one the same learned dynamics reaches with the
analytic reward.

    python examples/learned_reward_pendulum.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP   # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies import RandomPolicy                                   # noqa: E402
from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy                           # noqa: E402
from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP    # noqa: E402
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

reward_model = LearnedRewardMLP(dim_S=3, dim_U=1, layers=[64, 64, 1], activations=["tanh", "tanh", None], inputs="sas", seed=1)
handler = learn_dynamics_from_policy(
    env, RandomPolicy(num_agents, action_space, seed=0), number_of_rollouts=8, task_horizon=task_horizon,
    dynamics_function=DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=0),
    epochs=30, learning_rate=1e-3, batch_size=128, seed=0,
    reward_model=reward_model, reward_train_args=dict(epochs=30, learning_rate=1e-3, batch_size=128, seed=0))
print("dynamics: last validation loss %.4f; reward model: last validation loss %.4f (normalised targets)"
      % (handler.validation_loss[-1], reward_model.validation_loss[-1]))

returns = {}
for label, reward in (("learned reward", reward_model), ("analytic reward", pendulum_reward_function)):
    policy = MPCPolicy(reward_function=reward, env_action_space=action_space, env_observation_space=observation_space,
                       dynamics_handler=handler, optimizer_name="CEM", num_agents=num_agents, planning_horizon=30,
                       population_size=500, num_elite=50, max_iterations=5)
    obs, acs, rews = perform_rollouts(env, 1, task_horizon, policy)
    returns[label] = float(np.mean(np.sum(rews[0], axis=0)))
    print("CEM through the learned dynamics with the %-15s: mean closed-loop return %8.1f, upright at the end: %d/%d agents"
          % (label, returns[label], int(np.sum(obs[0][-1][:, 0] > 0.95)), num_agents))
