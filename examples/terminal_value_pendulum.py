"""Plan short, see far: a DeterministicMLP learns the pendulum's dynamics and a LearnedValueMLP the n-step return V(s)
from the same episodes; CEM then controls the real system at planning horizon 10 with w * V(s_H) closing every rollout,
next to horizon 10 without it and to horizon 30 without it (three times the model steps per candidate).

The value function is fitted on episodes of an MPC policy that plans at the long horizon through the learned model: what
V then holds is "what a good controller still collects from here".

    python examples/terminal_value_pendulum.py
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
from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.dynamics_learning import learn_dynamics_from_policy      # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402
from blackbox_mpc_amd.utils.rollouts import ModelEnvironment, perform_rollouts       # noqa: E402
from blackbox_mpc_amd.value_functions import LearnedValueMLP                         # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
N_STEP, GAMMA = 30, 0.97


def make_env(num_agents, seed=0):
    rng = np.random.default_rng(seed)
    theta0 = rng.uniform(-np.pi, np.pi, num_agents)
    start = np.stack([np.cos(theta0), np.sin(theta0), rng.uniform(-1, 1, num_agents)], axis=1).astype(np.float32)
    true_handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
    return ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)


def make_policy(handler, num_agents, horizon, value=None, weight=1.0):
    return MPCPolicy(reward_function=pendulum_reward_function, env_action_space=action_space,
                     env_observation_space=observation_space, dynamics_handler=handler, optimizer_name="CEM",
                     num_agents=num_agents, planning_horizon=horizon, population_size=500, num_elite=50, max_iterations=5,
                     terminal_value=value, terminal_weight=weight)


def learn(env, num_agents, task_horizon, seed=0):
    """(handler, value): dynamics from random-policy episodes, V from episodes of the long-horizon controller"""
    handler = learn_dynamics_from_policy(
        env, RandomPolicy(num_agents, action_space, seed=seed), number_of_rollouts=8, task_horizon=task_horizon,
        dynamics_function=DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=seed),
        epochs=30, learning_rate=1e-3, batch_size=128, seed=seed)
    value = LearnedValueMLP(dim_S=3, layers=[64, 64, 1], activations=["tanh", "tanh", None], seed=seed + 1)
    teacher = make_policy(handler, num_agents, 30)
    traj_obs, _, traj_rews = perform_rollouts(env, 2, task_horizon, teacher)
    value.train_on_rollouts(traj_obs, traj_rews, N_STEP, gamma=GAMMA, epochs=60, learning_rate=1e-3, batch_size=128, seed=seed)
    return handler, value


def closed_loop_return(env, policy, task_horizon):
    obs, _, rews = perform_rollouts(env, 1, task_horizon, policy)
    return float(np.mean(np.sum(rews[0], axis=0))), int(np.sum(obs[0][-1][:, 0] > 0.95))


if __name__ == "__main__":
    num_agents, task_horizon = 10, 200
    env = make_env(num_agents)
    handler, value = learn(env, num_agents, task_horizon)
    print("dynamics: last validation loss %.4f; value model: last validation loss %.4f (normalised targets)"
          % (handler.validation_loss[-1], value.validation_loss[-1]))
    for label, horizon, v in (("H = 30, no V", 30, None), ("H = 10, no V", 10, None), ("H = 10, V", 10, value)):
        ret, up = closed_loop_return(env, make_policy(handler, num_agents, horizon, v), task_horizon)
        print("CEM through the learned dynamics, %-13s: mean closed-loop return %8.1f, upright at the end: %d/%d agents"
              % (label, ret, up, num_agents))
