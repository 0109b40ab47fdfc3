"""Plan through a learned pendulum model that knows what it does not know: a bootstrap ensemble of three networks is
fitted on random-policy episodes -- which rarely visit the upright region the controller wants to reach -- and the
particle planner rolls particle p of every candidate through member p mod 3 for the whole horizon (trajectory
sampling).  Where the members disagree the per-particle returns spread, and mean - kappa * std steers the plan away
from candidates that only look good to one model.  The single-model planner on member 0 is run for comparison; both
control the true pendulum.

    python examples/ensemble_pendulum.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_functions import EnsembleMLP                          # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies import MPCPolicy                                      # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator, ParticleTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
plant = DeterministicTrajectoryEvaluator(pendulum_reward_function,
                                         SystemDynamicsHandler(action_space, observation_space,
                                                               dynamics_function=PendulumTrueModel(), true_model=True))

# ---- random-policy episodes from the true pendulum: observations [T+1, A, S], actions [T, A, U] per episode
rng = np.random.default_rng(0)
episodes, steps_per_episode = 20, 100
observations, actions, rewards = [], [], []
for _ in range(episodes):
    theta = rng.uniform(-np.pi, np.pi)
    obs = np.array([[np.cos(theta), np.sin(theta), rng.uniform(-1.0, 1.0)]], np.float32)
    ep_obs, ep_act, ep_rew = [obs], [], []
    for _ in range(steps_per_episode):
        act = rng.uniform(-2.0, 2.0, (1, 1)).astype(np.float32)
        nxt = plant.predict_next_state(obs, act)
        ep_rew.append(plant.evaluate_next_reward(obs, nxt, act))
        ep_obs.append(nxt)
        ep_act.append(act)
        obs = nxt
    observations.append(np.array(ep_obs))
    actions.append(np.array(ep_act))
    rewards.append(np.array(ep_rew))

# ---- a 3-member ensemble, each member on its own bootstrap resample of the training rows
model = EnsembleMLP([4, 32, 32, 32, 3], ["tanh", "tanh", "tanh", None], num_members=3, seed=0)
handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=model, is_normalized=True)
handler.train(observations, actions, rewards, validation_split=0.2, batch_size=128, learning_rate=1e-3, epochs=30, seed=0)
print("validation loss per member:", ["%.2e" % v[-1] for v in handler.member_validation_loss])
print("one-step residual (RMS over members):", handler.residual_std())

evaluators = {
    "member 0 alone": DeterministicTrajectoryEvaluator(pendulum_reward_function, handler),
    "ensemble (P=6, E=3, kappa=1)": ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=6,
                                                                process_noise_std=handler.residual_std(), risk_kappa=1.0),
}
steps = 150
for name, evaluator in evaluators.items():
    policy = MPCPolicy(trajectory_evaluator=evaluator, env_action_space=action_space, env_observation_space=observation_space,
                       optimizer_name="CEM", num_agents=1, planning_horizon=30, population_size=500, max_iterations=5,
                       num_elite=50, seed=0)
    obs = np.array([-1.0, 0.0, 0.0], np.float32)         # hanging down
    total = 0.0
    for t in range(steps):
        action, _, _ = policy.act(obs, t)
        nxt = plant.predict_next_state(obs[None], action[None])[0]
        total += float(plant.evaluate_next_reward(obs[None], nxt[None], action[None])[0])
        obs = nxt
    print("%-30s return over %d steps: %9.2f   final angle %.3f rad" % (name, steps, total, np.arctan2(obs[1], obs[0])))
