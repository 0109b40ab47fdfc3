"""A distilled policy among CEM's candidates: a DeterministicMLP learns the pendulum's dynamics, a LearnedValueMLP the n-step
return and a LearnedPolicyMLP the actions a long-horizon, large-population controller executed (behaviour cloning).  CEM then
controls the real system at planning horizon 10 with w * V(s_H) closing every rollout, at populations 500 and 50, with and
without the policy's closed-loop rollouts among the candidates of every iteration.

    python examples/policy_prior_pendulum.py
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
from blackbox_mpc_amd.policy_functions import LearnedPolicyMLP                       # noqa: E402
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


def make_policy(handler, num_agents, horizon, population, value=None, prior=None, prior_candidates=0, prior_std=0.0, seed=0):
    elite = max(5, population // 10)
    return MPCPolicy(reward_function=pendulum_reward_function, env_action_space=action_space,
                     env_observation_space=observation_space, dynamics_handler=handler, optimizer_name="CEM",
                     num_agents=num_agents, planning_horizon=horizon, population_size=population, num_elite=elite,
                     max_iterations=5, terminal_value=value, policy_prior=prior, prior_candidates=prior_candidates,
                     prior_std=prior_std, seed=seed)


def learn(env, num_agents, task_horizon, seed=0):
    """(handler, value, policy): dynamics from random-policy episodes; V and the policy from episodes of the long-horizon,
    large-population controller"""
    handler = learn_dynamics_from_policy(
        env, RandomPolicy(num_agents, action_space, seed=seed), number_of_rollouts=8, task_horizon=task_horizon,
        dynamics_function=DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=seed),
        epochs=30, learning_rate=1e-3, batch_size=128, seed=seed)
    value = LearnedValueMLP(dim_S=3, layers=[64, 64, 1], activations=["tanh", "tanh", None], seed=seed + 1)
    policy = LearnedPolicyMLP(dim_S=3, dim_U=1, layers=[64, 64, 1], activations=["tanh", "tanh", None], seed=seed + 2)
    teacher = make_policy(handler, num_agents, 30, 500)
    traj_obs, traj_acs, traj_rews = perform_rollouts(env, 2, task_horizon, teacher)
    value.train_on_rollouts(traj_obs, traj_rews, N_STEP, gamma=GAMMA, epochs=60, learning_rate=1e-3, batch_size=128, seed=seed)
    policy.train_on_rollouts(traj_obs, traj_acs, epochs=60, learning_rate=1e-3, batch_size=128, seed=seed)
    return handler, value, policy


def closed_loop_return(env, policy, task_horizon):
    obs, _, rews = perform_rollouts(env, 1, task_horizon, policy)
    return float(np.mean(np.sum(rews[0], axis=0))), int(np.sum(obs[0][-1][:, 0] > 0.95))


if __name__ == "__main__":
    num_agents, task_horizon = 10, 200
    env = make_env(num_agents)
    handler, value, prior = learn(env, num_agents, task_horizon)
    print("dynamics: last validation loss %.4f; value: %.4f; policy: %.4f (normalised targets)"
          % (handler.validation_loss[-1], value.validation_loss[-1], prior.validation_loss[-1]))
    for population in (500, 50):
        for label, net in (("no prior", None), ("8 policy rollouts", prior)):
            pol = make_policy(handler, num_agents, 10, population, value, net, 8 if net is not None else 0, 0.3)
            ret, up = closed_loop_return(env, pol, task_horizon)
            print("CEM, H = 10 + V, population %3d, %-17s: mean closed-loop return %8.1f, upright at the end: %d/%d agents"
                  % (population, label, ret, up, num_agents))
