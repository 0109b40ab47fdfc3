"""PETS with a cost of your own: a 3-member bootstrap ensemble fitted to random-policy data from the pendulum (as in
examples/ensemble_pendulum.py), and a reward written as HIP source with one runtime parameter per agent -- the angle the
agent should hold.  Every candidate is rolled out 6 times through the ensemble (trajectory sampling) with the measured
one-step residual as process noise, the user's reward scores every particle, and the candidates are ranked by the mean
of their 2 worst returns (CVaR, as in examples/cvar_pendulum.py).  Changing the goals is an upload, never a recompile.

    python examples/pets_custom_reward.py
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
from blackbox_mpc_amd.utils.device_functions import HipRewardFunction                # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402

# reward(current_state, actions, next_state) per row; params: this agent's row [goal angle], t: the planning step
HOLD_ANGLE = """
__device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,
                                          const float* params, int t) {
    const float err = atan2f(nxt[1], nxt[0]) - params[0];
    const float wrapped = atan2f(sinf(err), cosf(err));
    return -(wrapped * wrapped) - 0.1f * (nxt[2] * nxt[2]) - 0.001f * (act[0] * act[0]);
}
"""

action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
plant = DeterministicTrajectoryEvaluator(pendulum_reward_function,
                                         SystemDynamicsHandler(action_space, observation_space,
                                                               dynamics_function=PendulumTrueModel(), true_model=True))

# ---- random-policy episodes from the true pendulum: observations [T+1, A, S], actions [T, A, U] per episode
rng = np.random.default_rng(0)
observations, actions, rewards = [], [], []
for _ in range(20):
    theta = rng.uniform(-np.pi, np.pi)
    obs = np.array([[np.cos(theta), np.sin(theta), rng.uniform(-1.0, 1.0)]], np.float32)
    ep_obs, ep_act, ep_rew = [obs], [], []
    for _ in range(100):
        act = rng.uniform(-2.0, 2.0, (1, 1)).astype(np.float32)
        nxt = plant.predict_next_state(obs, act)
        ep_rew.append(plant.evaluate_next_reward(obs, nxt, act))
        ep_obs.append(nxt)
        ep_act.append(act)
        obs = nxt
    observations.append(np.array(ep_obs))
    actions.append(np.array(ep_act))
    rewards.append(np.array(ep_rew))

model = EnsembleMLP([4, 32, 32, 32, 3], ["tanh", "tanh", "tanh", None], num_members=3, seed=0)
handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=model, is_normalized=True)
handler.train(observations, actions, rewards, validation_split=0.2, batch_size=128, learning_rate=1e-3, epochs=30, seed=0)
sigma = handler.residual_std()
print("one-step residual (RMS over members, the process noise):", sigma)

num_agents, planning_horizon = 2, 20
reward = HipRewardFunction(HOLD_ANGLE, num_params=1)
reward.set_params(np.array([[0.0], [0.5]], np.float32))            # agent 0 holds upright, agent 1 half a radian off
evaluator = ParticleTrajectoryEvaluator(reward, handler, num_particles=6, process_noise_std=sigma, risk_alpha=1.0 / 3.0)
policy = MPCPolicy(trajectory_evaluator=evaluator, env_action_space=action_space, env_observation_space=observation_space,
                   optimizer_name="CEM", num_agents=num_agents, planning_horizon=planning_horizon, population_size=300,
                   num_elite=30, max_iterations=4, seed=0)
policy.keep_plan(True)
obs = np.tile(np.array([[np.cos(0.3), np.sin(0.3), 0.0]], np.float32), (num_agents, 1))
for t in range(60):
    if t == 30:
        reward.set_params(np.array([[0.5], [0.0]], np.float32))    # swap the goals: uploaded before the next step
    action, _, _ = policy.act(obs, t)
    obs = plant.predict_next_state(obs, action)
    if t % 10 == 9:
        print("step %2d: angles %s" % (t, np.round(np.arctan2(obs[:, 1], obs[:, 0]), 3)))
_, state_mean, state_std, reward_mean, reward_std, state_q, reward_q = policy.plan_distribution(obs, quantiles=[0.05, 0.95])
print("agent 0, predicted reward along the plan:  step   5 %     mean    95 %")
for t in range(0, planning_horizon, 4):
    print("                                           %3d  %7.3f %7.3f %7.3f" % (t, reward_q[0, 0, t], reward_mean[0, t], reward_q[0, 1, t]))
