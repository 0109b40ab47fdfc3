"""Sample, then follow the gradient: a DeterministicMLP learns the pendulum's dynamics and a LearnedRewardMLP its reward
from the same random-policy episodes; CEM plans through both networks, and MPCPolicy(refine_steps=3) then improves CEM's
plan by three projected gradient steps on the model return (Engine.plan_gradient: the derivative of the return in every
action, through both networks, in one kernel launch) before it acts.  The closed-loop return on the real system is
printed with and without the refinement, for a small and for a larger CEM population.

    python examples/plan_gradient_pendulum.py
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


def make_env(num_agents, seed=0):
    rng = np.random.default_rng(seed)
    theta0 = rng.uniform(-np.pi, np.pi, num_agents)
    start = np.stack([np.cos(theta0), np.sin(theta0), rng.uniform(-1, 1, num_agents)], axis=1).astype(np.float32)
    true_handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
    return ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)


def learn(env, num_agents, task_horizon, seed=0):
    """(handler, reward_model) from random-policy episodes"""
    reward_model = LearnedRewardMLP(dim_S=3, dim_U=1, layers=[64, 64, 1], activations=["tanh", "tanh", None], inputs="sas", seed=seed + 1)
    handler = learn_dynamics_from_policy(
        env, RandomPolicy(num_agents, action_space, seed=seed), number_of_rollouts=8, task_horizon=task_horizon,
        dynamics_function=DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=seed),
        epochs=30, learning_rate=1e-3, batch_size=128, seed=seed,
        reward_model=reward_model, reward_train_args=dict(epochs=30, learning_rate=1e-3, batch_size=128, seed=seed))
    return handler, reward_model


def make_policy(handler, reward_model, num_agents, population, refine_steps):
    return MPCPolicy(reward_function=reward_model, env_action_space=action_space, env_observation_space=observation_space,
                     dynamics_handler=handler, optimizer_name="CEM", num_agents=num_agents, planning_horizon=30,
                     population_size=population, num_elite=max(4, population // 10), max_iterations=5, refine_steps=refine_steps,
                     refine_lr=0.05)


def closed_loop_return(env, policy, task_horizon):
    obs, _, rews = perform_rollouts(env, 1, task_horizon, policy)
    return float(np.mean(np.sum(rews[0], axis=0))), int(np.sum(obs[0][-1][:, 0] > 0.95))


if __name__ == "__main__":
    num_agents, task_horizon = 10, 200
    env = make_env(num_agents)
    handler, reward_model = learn(env, num_agents, task_horizon)
    print("dynamics: last validation loss %.4f; reward model: last validation loss %.4f (normalised targets)"
          % (handler.validation_loss[-1], reward_model.validation_loss[-1]))
    for population in (50, 500):
        for steps in (0, 3):
            ret, up = closed_loop_return(env, make_policy(handler, reward_model, num_agents, population, steps), task_horizon)
            print("CEM N = %3d through the learned networks, refine_steps = %d: mean closed-loop return %8.1f, upright at the end: %d/%d agents"
                  % (population, steps, ret, up, num_agents))
