"""Temporally correlated ("colored") sampling: the true-model pendulum tutorial of examples/true_model_mpc.py with
noise_beta = 2.0 -- every candidate action sequence of CEM / PI2 is drawn with iCEM's power-law noise (red noise: the
draws of neighbouring planning steps are correlated, so a candidate holds a torque long enough to swing the pendulum)
instead of independently per step -- next to the white-noise default, at a small population.

    python examples/colored_noise_pendulum.py    # needs an MI355X and the built libbbmpc.so
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy                            # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.colored_noise import ar1_mixing, colored_noise_mixing    # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402
from blackbox_mpc_amd.utils.rollouts import ModelEnvironment, perform_rollouts       # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
num_agents, task_horizon, planning_horizon = 4, 200, 30

# hanging down (theta = pi), at rest: the swing-up task
start = np.tile(np.array([[-1.0, 0.0, 0.0]], np.float32), (num_agents, 1))
handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, handler), start)

print("lag-1 correlation of the draws: beta 0 -> %.2f, beta 1 -> %.2f, beta 2 -> %.2f"
      % tuple(colored_noise_mixing(planning_horizon, b)[1, 0] for b in (0.0, 1.0, 2.0)))
for name, kwargs in [("CEM", dict(population_size=64, num_elite=8, max_iterations=3)),
                     ("PI2", dict(population_size=64, max_iterations=3))]:
    for label, extra in [("white (default)", {}), ("noise_beta=2.0", dict(noise_beta=2.0)),
                         ("AR(1), rho=0.9", dict(sampling_correlation=ar1_mixing(planning_horizon, 0.9)))]:
        mpc_policy = MPCPolicy(reward_function=pendulum_reward_function, env_action_space=action_space,
                               env_observation_space=observation_space, true_model=True,
                               dynamics_function=PendulumTrueModel(), optimizer_name=name, num_agents=num_agents,
                               planning_horizon=planning_horizon, seed=0, **kwargs, **extra)
        traj_obs, traj_acs, traj_rews = perform_rollouts(env, 1, task_horizon, mpc_policy)
        final_cos = traj_obs[0][-1][:, 0]
        print("%-4s %-16s episode reward %8.1f   upright at the end: %d/%d agents"
              % (name, label, float(np.mean(np.sum(traj_rews[0], axis=0))), int(np.sum(final_cos > 0.95)), num_agents))
