"""PETS' probabilistic ensemble fitted by the hand-written training kernels in ONE launch sequence, then planned through:
`backend="hip_nll"` sends the members of an EnsembleMLP(probabilistic=True) -- mean network and log-variance head each -- to
one HipGaussianEnsembleTrainer (bbmpc_trainer_create_gaussian / bbmpc_trainer_fit_ensemble).  The loss is the Gaussian
negative log-likelihood, the member index is a grid dimension of the training kernels, the rows are on the device once and a
member's bootstrap resample is an index map.  The fitted ensemble is what the particle evaluator plans through: particle p
follows member p mod E for the whole horizon and draws its process noise from that member's learned variance.

    python examples/train_hip_probabilistic_ensemble_pendulum.py            # 5 members, 30 epochs, 60 control steps
    python examples/train_hip_probabilistic_ensemble_pendulum.py --small    # a few seconds: 3 members, fewer rows, epochs, steps
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_functions import EnsembleMLP                          # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.policies import MPCPolicy                                      # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator, ParticleTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402

small = "--small" in sys.argv
action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
plant = DeterministicTrajectoryEvaluator(pendulum_reward_function,
                                         SystemDynamicsHandler(action_space, observation_space,
                                                               dynamics_function=PendulumTrueModel(), true_model=True))

# ---- random-policy episodes from the true pendulum: observations [T+1, A, S], actions [T, A, U] per episode
rng = np.random.default_rng(0)
episodes, steps_per_episode = (6, 50) if small else (20, 100)
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

# ---- the probabilistic ensemble: every member on its own bootstrap resample, mean and head, all of them in one fit
members, epochs, batch_size = (3, 5, 32) if small else (5, 30, 128)
model = EnsembleMLP([4, 32, 32, 32, 3], ["tanh", "tanh", "tanh", None], num_members=members, seed=0, probabilistic=True)
handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=model, is_normalized=True)
t0 = time.perf_counter()
handler.train(observations, actions, rewards, validation_split=0.2, batch_size=batch_size, learning_rate=1e-3, epochs=epochs, seed=0,
              backend="hip_nll")
print("%d members, %d epochs on %d rows in %.2f s (one HIP Gaussian ensemble fit); validation NLL per member, first -> last epoch: %s"
      % (members, epochs, handler._model_training_in.shape[0], time.perf_counter() - t0,
         ["%.3f -> %.3f" % (v[0], v[-1]) for v in handler.member_validation_loss]))
print("one-step residual of the mean networks (RMS over members):", handler.residual_std())

# ---- a few control steps through the ensemble on the true pendulum: the noise is the members' learned variance
evaluator = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=2 * members, process_noise_std=0.0,
                                        risk_kappa=1.0)
policy = MPCPolicy(trajectory_evaluator=evaluator, env_action_space=action_space, env_observation_space=observation_space,
                   optimizer_name="CEM", num_agents=1, planning_horizon=10 if small else 30, population_size=64 if small else 500,
                   max_iterations=2 if small else 5, num_elite=8 if small else 50, seed=0)
obs = np.array([-1.0, 0.0, 0.0], np.float32)             # hanging down
steps, total = (5 if small else 60), 0.0
for t in range(steps):
    action, _, _ = policy.act(obs, t)
    nxt = plant.predict_next_state(obs[None], action[None])[0]
    total += float(plant.evaluate_next_reward(obs[None], nxt[None], action[None])[0])
    obs = nxt
print("planned %d control steps through the ensemble: return %.2f, angle now %.3f rad" % (steps, total, np.arctan2(obs[1], obs[0])))
