"""Plan around an episode end: the pendulum with a speed limit.  A DeterministicMLP learns the dynamics; the task ends,
at a cost, when |thdot| leaves a box on state index 2.  CEM plans through the learned model with discount 0.99, a
LearnedValueMLP fitted with the same gamma (its n-step windows stop where the box says the episode ends), and the
StateBoxTermination with a negative terminal reward -- next to the same planner without the termination.  Both control the
analytic pendulum as the real system; printed is the share of executed steps that violate the box, and the return.

    python examples/termination_pendulum.py
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
from blackbox_mpc_amd.utils.termination import StateBoxTermination                   # noqa: E402
from blackbox_mpc_amd.value_functions import LearnedValueMLP                         # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
N_STEP, GAMMA, SPEED_LIMIT, TERMINAL_REWARD, HORIZON = 15, 0.99, 5.0, -100.0, 15


def speed_box():
    return StateBoxTermination(low=[-np.inf, -np.inf, -SPEED_LIMIT], high=[np.inf, np.inf, SPEED_LIMIT], terminal_reward=TERMINAL_REWARD)


def make_env(num_agents, seed=0):
    rng = np.random.default_rng(seed)
    theta0 = rng.uniform(-np.pi, np.pi, num_agents)
    start = np.stack([np.cos(theta0), np.sin(theta0), rng.uniform(-1, 1, num_agents)], axis=1).astype(np.float32)
    true_handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
    return ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)


def make_policy(handler, num_agents, value=None, box=None, discount=GAMMA):
    return MPCPolicy(reward_function=pendulum_reward_function, env_action_space=action_space,
                     env_observation_space=observation_space, dynamics_handler=handler, optimizer_name="CEM",
                     num_agents=num_agents, planning_horizon=HORIZON, population_size=500, num_elite=50, max_iterations=5,
                     terminal_value=value, discount=discount, termination=box)


def learn(env, num_agents, task_horizon, box, seed=0):
    """(handler, value): dynamics from random-policy episodes; V from episodes of the planner without a value, its windows
    cut where the box ends the episode"""
    handler = learn_dynamics_from_policy(
        env, RandomPolicy(num_agents, action_space, seed=seed), number_of_rollouts=8, task_horizon=task_horizon,
        dynamics_function=DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=seed),
        epochs=30, learning_rate=1e-3, batch_size=128, seed=seed)
    value = LearnedValueMLP(dim_S=3, layers=[64, 64, 1], activations=["tanh", "tanh", None], seed=seed + 1)
    teacher = make_policy(handler, num_agents, None, box)
    traj_obs, _, traj_rews = perform_rollouts(env, 2, task_horizon, teacher)
    done = [box(np.asarray(o)[1:]) for o in traj_obs]
    value.train_on_rollouts(traj_obs, traj_rews, N_STEP, gamma=GAMMA, terminated=done, epochs=60, learning_rate=1e-3, batch_size=128, seed=seed)
    return handler, value


def violation_share_and_return(env, policy, task_horizon, box):
    """(share of executed steps whose state lies outside the box, mean undiscounted return over the agents)"""
    obs, _, rews = perform_rollouts(env, 1, task_horizon, policy)
    return float(np.mean(box(np.asarray(obs[0])[1:]))), float(np.mean(np.sum(rews[0], axis=0)))


if __name__ == "__main__":
    num_agents, task_horizon = 10, 200
    env, box = make_env(num_agents), speed_box()
    handler, value = learn(env, num_agents, task_horizon, box)
    print("dynamics: last validation loss %.4f; value model: last validation loss %.4f (normalised targets)"
          % (handler.validation_loss[-1], value.validation_loss[-1]))
    for label, b in (("discount %.2f, V, no termination" % GAMMA, None), ("discount %.2f, V, |thdot| <= %.0f (c = %.0f)" % (GAMMA, SPEED_LIMIT, TERMINAL_REWARD), box)):
        share, ret = violation_share_and_return(env, make_policy(handler, num_agents, value, b), task_horizon, box)
        print("CEM through the learned dynamics, %-42s: %5.1f %% of the executed steps outside the box, mean return %8.1f" % (label, 100 * share, ret))
