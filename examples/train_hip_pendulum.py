"""The iterative-MPC tutorial (examples/learn_dynamics_and_control.py) with every fit done by the hand-written training
kernels: `backend="hip"` in `train_args` sends SystemDynamicsHandler.train to HipDenseTrainer (bbmpc_trainer_*: forward,
backward and the Adam update of a mini-batch in two kernel launches) instead of the torch DenseTrainer.  Nothing else
changes: the same split, statistics and epochs, the planner picks the refitted weights up as before.

    python examples/train_hip_pendulum.py            # the tutorial's sizes
    python examples/train_hip_pendulum.py --small    # a few seconds: fewer agents, rollouts and epochs
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP   # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies import RandomPolicy                                   # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.iterative_mpc import learn_dynamics_iteratively_w_mpc    # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402
from blackbox_mpc_amd.utils.rollouts import ModelEnvironment, perform_rollouts       # noqa: E402

small = "--small" in sys.argv
action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
num_agents, task_horizon = (4, 40) if small else (10, 200)

rng = np.random.default_rng(0)
theta0 = rng.uniform(-np.pi, np.pi, num_agents)
start = np.stack([np.cos(theta0), np.sin(theta0), rng.uniform(-1, 1, num_agents)], axis=1).astype(np.float32)
true_handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)

dynamics_function = DeterministicMLP(layers=[4, 32, 32, 32, 3], activation_functions=["tanh", "tanh", "tanh", None], seed=0)
t0 = time.perf_counter()
handler, mpc_policy = learn_dynamics_iteratively_w_mpc(
    env, number_of_initial_rollouts=3 if small else 5, number_of_rollouts_for_refinement=1 if small else 2,
    number_of_refinement_steps=1 if small else 3,
    task_horizon=task_horizon, env_action_space=action_space, env_observation_space=observation_space,
    initial_policy=RandomPolicy(num_agents, action_space, seed=0), planning_horizon=10 if small else 30,
    reward_function=pendulum_reward_function, optimizer_name="CEM", num_agents=num_agents,
    dynamics_function=dynamics_function, epochs=5 if small else 30, learning_rate=1e-3, batch_size=32 if small else 128,
    train_args={"seed": 0, "backend": "hip"},
    population_size=64 if small else 500, num_elite=8 if small else 50, max_iterations=2 if small else 5)
print("transitions collected: %d train + %d validation; last validation loss %.4f  (%.1f s, fits by the HIP trainer)"
      % (handler._model_training_in.shape[0], handler._model_validation_in.shape[0], handler.validation_loss[-1],
         time.perf_counter() - t0))

traj_obs, traj_acs, traj_rews = perform_rollouts(env, 1, task_horizon, mpc_policy)
print("MPC through the learned model on the real system: mean episode reward %.1f, upright at the end: %d/%d agents"
      % (float(np.mean(np.sum(traj_rews[0], axis=0))), int(np.sum(traj_obs[0][-1][:, 0] > 0.95)), num_agents))
