"""Swing the pendulum up while the real system's actuation is noisy: the plant adds a random torque disturbance every
step, which shows up as noise on the angular velocity the model did not predict.  A deterministic planner scores each
candidate by one noise-free rollout; the particle planner rolls it out under sampled process noise and penalises
candidates whose return varies (mean - kappa * std).  Both control the same noisy plant with the same disturbances.

    python examples/pendulum_actuation_noise.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies import MPCPolicy                                      # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator, ParticleTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=PendulumTrueModel(), true_model=True)
torque_noise_std = 1.0                                   # N m; thdot changes by 3 * torque * dt = 0.15 per unit of torque
thdot_std = 3.0 * torque_noise_std * 0.05
steps = 150

evaluators = {
    "deterministic": DeterministicTrajectoryEvaluator(pendulum_reward_function, handler),
    "particles (P=8, kappa=1)": ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=8,
                                                            process_noise_std=[0.0, 0.0, thdot_std], risk_kappa=1.0),
}
plant = DeterministicTrajectoryEvaluator(pendulum_reward_function, handler)
for name, evaluator in evaluators.items():
    policy = MPCPolicy(trajectory_evaluator=evaluator, env_action_space=action_space, env_observation_space=observation_space,
                       optimizer_name="CEM", num_agents=1, planning_horizon=30, population_size=500, max_iterations=5,
                       num_elite=50, seed=0)
    rng = np.random.default_rng(1)                       # the same disturbances for both planners
    obs = np.array([-1.0, 0.0, 0.0], np.float32)         # hanging down
    total = 0.0
    for t in range(steps):
        action, _, _ = policy.act(obs, t)
        applied = action + rng.normal(0.0, torque_noise_std, 1).astype(np.float32)
        nxt = plant.predict_next_state(obs[None], applied[None])[0]
        total += float(plant.evaluate_next_reward(obs[None], nxt[None], action[None])[0])
        obs = nxt
    print("%-26s return over %d noisy steps: %9.2f   final angle %.3f rad" % (name, steps, total, np.arctan2(obs[1], obs[0])))
