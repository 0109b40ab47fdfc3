"""A bootstrap ensemble on FEW rows -- the first rounds of an iterative-MPC loop -- fitted the way PETS and MBPO fit
theirs: per-layer weight decay, every member stopped on its own holdout loss, the best holdout weights kept.  All of it runs
inside the one HIP ensemble fit: the decay in the update kernel, the stopping decision and the
snapshot of the best weights in a monitor launch per epoch, no host synchronisation before the end.  Without them the
members overfit a few hundred rows and their disagreement -- what mean - kappa * std plans on -- is mostly noise.

    python examples/train_regularized_ensemble_pendulum.py            # 5 members, up to 200 epochs on 300 rows
    python examples/train_regularized_ensemble_pendulum.py --small    # a few seconds: 3 members, up to 40 epochs
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd import Box                                                     # noqa: E402
from blackbox_mpc_amd.dynamics_functions import EnsembleMLP                          # noqa: E402
from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler   # noqa: E402
from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator  # noqa: E402
from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function  # noqa: E402

small = "--small" in sys.argv
action_space = Box(low=[-2.0], high=[2.0])
observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
plant = DeterministicTrajectoryEvaluator(pendulum_reward_function,
                                         SystemDynamicsHandler(action_space, observation_space,
                                                               dynamics_function=PendulumTrueModel(), true_model=True))

# ---- three short random-policy episodes: observations [T+1, A, S], actions [T, A, U] per episode
rng = np.random.default_rng(0)
observations, actions, rewards = [], [], []
for _ in range(3):
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

members, epochs = (3, 40) if small else (5, 200)
layers, acts = [4, 64, 64, 3], ["swish", "swish", None]


def fit(**options):
    model = EnsembleMLP(layers, acts, num_members=members, seed=0)
    handler = SystemDynamicsHandler(action_space, observation_space, dynamics_function=model, is_normalized=True)
    t0 = time.perf_counter()
    handler.train(observations, actions, rewards, validation_split=0.25, batch_size=32, learning_rate=3e-3, epochs=epochs, seed=0,
                  backend="hip", **options)
    return handler, time.perf_counter() - t0


plain, t_plain = fit()
reg, t_reg = fit(weight_decay=[2.5e-5, 5e-5, 7.5e-5],         # PETS: a larger lambda towards the output
                 decay_mode="l2", patience=10, restore_best=True)
print("%d members on %d training rows, up to %d epochs" % (members, reg._model_training_in.shape[0], epochs))
print("  plain fit        %.2f s: every member ran %d epochs; final validation loss per member: %s"
      % (t_plain, epochs, ["%.2e" % v[-1] for v in plain.member_validation_loss]))
print("  decay + stopping %.2f s: best epoch per member %s, epochs run %s; validation loss kept: %s"
      % (t_reg, reg.member_best_epoch, reg.member_epochs_run,
         ["%.2e" % v[b] for v, b in zip(reg.member_validation_loss, reg.member_best_epoch)]))
print("  one-step residual (RMS over members): plain %s, regularised %s" % (plain.residual_std(), reg.residual_std()))
