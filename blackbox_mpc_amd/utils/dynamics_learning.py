"""learn_dynamics_from_policy -- counterpart of the reference's utils/dynamics_learning.py:7-90: collect episodes
with a policy, then fit the dynamics model on them (SystemDynamicsHandler.train, on the GPU)."""
from ..dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
from .rollouts import perform_rollouts


def learn_dynamics_from_policy(env, policy, number_of_rollouts, task_horizon, dynamics_function=None,
                               system_dynamics_handler=None, epochs=30, learning_rate=1e-3, validation_split=0.2,
                               batch_size=128, is_normalized=True, nn_optimizer=None, tf_writer=None,
                               exploration_noise=False, log_dir=None, save_model_frequency=1, saved_model_dir=None,
                               start_episode=0, multistep_horizon=None, reward_model=None, reward_train_args=None,
                               value_model=None, value_n_step=10, value_train_args=None, policy_model=None, policy_train_args=None,
                               **train_args):
    """Same arguments as the reference; `train_args` (device=, seed=, backend="torch" | "hip" | "hip_nll", ...) are forwarded to `train`.
    `multistep_horizon`: when set, the fit is followed by one SystemDynamicsHandler.multistep_error call over that many
    steps on the episodes just collected (the train / validation split is per transition, so there is no held-out
    episode to use instead); the result stays on the handler as `multistep_rmse` -- a TRAINING-set figure, optimistic
    as a training loss is: call `handler.multistep_error` on fresh episodes for a validation figure.  None: nothing extra is computed.
    `reward_model`: a LearnedRewardMLP that is refitted, on every episode it has been given so far, from the rewards these
    rollouts collect anyway (`reward_train_args`: a dict forwarded to its `train`; default: epochs / batch_size /
    learning_rate / validation_split of this call).
    `value_model`: a LearnedValueMLP that is refitted beside them on the `value_n_step`-step returns of every episode it
    has been given so far (`value_train_args`: a dict forwarded to its `train_on_rollouts`: gamma=, bootstrap=, epochs=, ...).
    `policy_model`: a LearnedPolicyMLP that is refitted beside them on the (observation, executed action) pairs of every
    episode it has been given so far (`policy_train_args`: a dict forwarded to its `train_on_rollouts`)."""
    if system_dynamics_handler is None:
        system_dynamics_handler = SystemDynamicsHandler(env_action_space=env.action_space,
                                                        env_observation_space=env.observation_space,
                                                        true_model=False, dynamics_function=dynamics_function,
                                                        tf_writer=tf_writer, is_normalized=is_normalized,
                                                        log_dir=log_dir, save_model_frequency=save_model_frequency,
                                                        saved_model_dir=saved_model_dir)
    traj_obs, traj_acs, traj_rews = perform_rollouts(env, number_of_rollouts, task_horizon, policy,
                                                     exploration_noise=exploration_noise, tf_writer=tf_writer,
                                                     start_episode=start_episode)
    system_dynamics_handler.train(traj_obs, traj_acs, traj_rews, validation_split=validation_split,
                                  batch_size=batch_size, learning_rate=learning_rate, epochs=epochs,
                                  nn_optimizer=nn_optimizer, **train_args)
    if reward_model is not None:
        args = dict(epochs=epochs, batch_size=batch_size, learning_rate=learning_rate, validation_split=validation_split)
        args.update(reward_train_args or {})
        reward_model.train_on_rollouts(traj_obs, traj_acs, traj_rews, **args)
    if value_model is not None:
        args = dict(epochs=epochs, batch_size=batch_size, learning_rate=learning_rate, validation_split=validation_split)
        args.update(value_train_args or {})
        value_model.train_on_rollouts(traj_obs, traj_rews, value_n_step, **args)
    if policy_model is not None:
        args = dict(epochs=epochs, batch_size=batch_size, learning_rate=learning_rate, validation_split=validation_split)
        args.update(policy_train_args or {})
        policy_model.train_on_rollouts(traj_obs, traj_acs, **args)
    if multistep_horizon is not None:
        system_dynamics_handler.multistep_error(traj_obs, traj_acs, multistep_horizon)
    return system_dynamics_handler
