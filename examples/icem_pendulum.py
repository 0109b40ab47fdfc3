"""iCEM on the true-model pendulum: the colored-noise example of examples/colored_noise_pendulum.py with both halves of
iCEM switched on -- noise_beta = 2.0 (power-law noise along the planning horizon) and the elite carry-over: the best
keep_elites of an iteration are put back among the candidates of the next one, the best shift_elites of a control step,
moved one planning step forward, among the candidates of the next control step.  Nothing good that was found is lost
between iterations or control steps, which is what lets the population shrink.

    python examples/icem_pendulum.py    # needs an MI355X and the built libbbmpc.so
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy                            # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402
from blackbox_mpc_amd.utils.rollouts import ModelEnvironment, perform_rollouts       # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
num_agents, task_horizon, planning_horizon = 4, 200, 30

# hanging down (theta = pi), at rest: the swing-up task
start = np.tile(np.array([[-1.0, 0.0, 0.0]], np.float32), (num_agents, 1))
handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, handler), start)

for label, kwargs in [("CEM, white noise, N=64", dict(population_size=64, num_elite=8)),
                      ("noise_beta=2.0, N=64", dict(population_size=64, num_elite=8, noise_beta=2.0)),
                      ("iCEM, N=64", dict(population_size=64, num_elite=8, noise_beta=2.0, keep_elites=3, shift_elites=3)),
                      ("iCEM, N=24", dict(population_size=24, num_elite=6, noise_beta=2.0, keep_elites=2, shift_elites=2))]:
    mpc_policy = MPCPolicy(reward_function=pendulum_reward_function, env_action_space=action_space,
                           env_observation_space=observation_space, true_model=True, dynamics_function=PendulumTrueModel(),
                           optimizer_name="CEM", num_agents=num_agents, planning_horizon=planning_horizon, max_iterations=3,
                           seed=0, **kwargs)
    traj_obs, traj_acs, traj_rews = perform_rollouts(env, 1, task_horizon, mpc_policy)
    final_cos = traj_obs[0][-1][:, 0]
    print("%-26s episode reward %8.1f   upright at the end: %d/%d agents   elite carry (keep, shift, stored) = %s"
          % (label, float(np.mean(np.sum(traj_rews[0], axis=0))), int(np.sum(final_cos > 0.95)), num_agents,
             mpc_policy._optimizer._engine.elite_carry()))
