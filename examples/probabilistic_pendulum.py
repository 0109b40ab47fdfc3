"""Plan through a learned pendulum model that has learned where it is noisy: the plant's torque is disturbed four times
as hard while the pendulum is in its lower half as in its upper half, a ProbabilisticMLP -- a mean network plus a
log-variance head -- is fitted on random-policy episodes by the Gaussian negative log-likelihood, and the particle planner
adds the predicted, state-dependent noise to every rollout step (process_noise_std = 0: the learned noise alone).
The deterministic planner on the mean network is run for comparison; both control the disturbed pendulum.

    python examples/probabilistic_pendulum.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_functions import ProbabilisticMLP                     # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies import MPCPolicy                                      # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator, ParticleTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
plant = DeterministicTrajectoryEvaluator(pendulum_reward_function,
                                         SystemDynamicsHandler(action_space, observation_space,
                                                               dynamics_function=PendulumTrueModel(), true_model=True))
rng = np.random.default_rng(0)


def disturbed_step(obs, act):
    """The true pendulum with torque noise: std 0.8 in the lower half (cos theta < 0), 0.2 in the upper half."""
    std = np.where(obs[:, :1] < 0.0, 0.8, 0.2)
    return plant.predict_next_state(obs, (act + std * rng.standard_normal(act.shape)).astype(np.float32))


# ---- random-policy episodes: observations [T+1, A, S], actions [T, A, U] per episode
episodes, steps_per_episode = 30, 100
observations, actions, rewards = [], [], []
for _ in range(episodes):
    theta = rng.uniform(-np.pi, np.pi)
    obs = np.array([[np.cos(theta), np.sin(theta), rng.uniform(-1.0, 1.0)]], np.float32)
    ep_obs, ep_act, ep_rew = [obs], [], []
    for _ in range(steps_per_episode):
        act = rng.uniform(-2.0, 2.0, (1, 1)).astype(np.float32)
        nxt = disturbed_step(obs, act)
        ep_rew.append(plant.evaluate_next_reward(obs, nxt, act))
        ep_obs.append(nxt)
        ep_act.append(act)
        obs = nxt
    observations.append(np.array(ep_obs))
    actions.append(np.array(ep_act))
    rewards.append(np.array(ep_rew))

model = ProbabilisticMLP([4, 32, 32, 32, 3], ["tanh", "tanh", "tanh", None], seed=0)
handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=model, is_normalized=True)
handler.train(observations, actions, rewards, validation_split=0.2, batch_size=128, learning_rate=1e-3, epochs=40, seed=0)
print("validation NLL, first and last epoch: %.3f -> %.3f" % (handler.validation_loss[0], handler.validation_loss[-1]))
print("one-step residual of the mean network:", handler.residual_std())

evaluators = {
    "mean network alone": DeterministicTrajectoryEvaluator(pendulum_reward_function, handler),
    "learned noise (P=8, kappa=1)": ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=8,
                                                                process_noise_std=0.0, risk_kappa=1.0),
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
        nxt = disturbed_step(obs[None], action[None])[0]
        total += float(plant.evaluate_next_reward(obs[None], nxt[None], action[None])[0])
        obs = nxt
    print("%-30s return over %d steps: %9.2f   final angle %.3f rad" % (name, steps, total, np.arctan2(obs[1], obs[0])))
