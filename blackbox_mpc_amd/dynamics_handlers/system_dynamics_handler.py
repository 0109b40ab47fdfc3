"""Counterpart of the reference's SystemDynamicsHandler (dynamics_handlers/system_dynamics_handler.py).

Inference half (:7-161): which dynamics function, whether it is the true model, and the six normalisation
statistics; process_input / process_output are fused into the rollout kernels (GEMM-1 prologue / GEMM-3 epilogue).
Training half (:163-349): dataset assembly, train/validation split, freeze-after-first
normalisation, shuffled drop-remainder batches, MSE + Keras-Adam on the GPU (dynamics_functions/_train_torch.py);
the SavedModel checkpoint is replaced by `mlp.npz` + the reference's six `.npy` statistics files."""
import os

import numpy as np

_STATS = ("mean_states", "std_states", "mean_actions", "std_actions", "mean_targets", "std_targets")


def multistep_windows(observations_trajectories, actions_trajectories, horizon, stride=1):
    """Cut every window of `horizon` steps out of episodes in train()'s layout (observations [T+1, A, S], actions
    [T, A, U] per episode): episode-major, then agent, then start t0 = 0, stride, 2 stride, ...; a window that would run
    past the end of its episode is dropped (an episode shorter than the horizon gives none).  Returns
    (start_states [B,S], actions [B,horizon,U], observed [B,horizon,S]) with observed[b, t] the recorded state t + 1 steps
    after the window's start."""
    horizon, stride = int(horizon), int(stride)
    if horizon < 1 or stride < 1:
        raise ValueError("horizon and stride must be >= 1")
    starts, acts, obs_w = [], [], []
    dim_s = dim_u = None
    for obs, acs in zip(observations_trajectories, actions_trajectories):
        obs, acs = np.asarray(obs, np.float32), np.asarray(acs, np.float32)
        if obs.ndim != 3 or acs.ndim != 3 or obs.shape[0] != acs.shape[0] + 1 or obs.shape[1] != acs.shape[1]:
            raise ValueError("an episode is observations [T+1, A, S] with actions [T, A, U], got %s and %s" % (obs.shape, acs.shape))
        dim_s, dim_u = obs.shape[2], acs.shape[2]
        steps = acs.shape[0]
        t0 = np.arange(0, steps - horizon + 1, stride)
        if t0.size == 0:
            continue
        idx = t0[:, None] + np.arange(horizon)[None, :]                 # [W, horizon]
        for agent in range(acs.shape[1]):
            starts.append(obs[t0, agent])
            acts.append(acs[idx, agent])
            obs_w.append(obs[idx + 1, agent])
    if not starts:
        return (np.zeros((0, dim_s or 0), np.float32), np.zeros((0, horizon, dim_u or 0), np.float32),
                np.zeros((0, horizon, dim_s or 0), np.float32))
    return (np.ascontiguousarray(np.concatenate(starts, axis=0)), np.ascontiguousarray(np.concatenate(acts, axis=0)),
            np.ascontiguousarray(np.concatenate(obs_w, axis=0)))


def calibration_z_rms(mean, std, observed):
    """RMS over the windows of the standardised error of a predicted distribution: mean / std / observed [W, horizon, S]
    -> z_rms [horizon, S] = sqrt(mean_w(((observed - mean) / max(std, 1e-12))^2)), in float64.  About 1 where the
    predicted spread is honest, above 1 where it is too narrow (std = 0 against a wrong mean gives a huge value, not a
    division by zero), below 1 where it is too wide."""
    mean, std, observed = (np.asarray(v, np.float64) for v in (mean, std, observed))
    if mean.ndim != 3 or mean.shape != std.shape or mean.shape != observed.shape:
        raise ValueError("mean, std and observed must be equal [W, horizon, S] arrays, got %s, %s, %s"
                         % (mean.shape, std.shape, observed.shape))
    if mean.shape[0] == 0:
        raise ValueError("calibration_z_rms: no window")
    z = (observed - mean) / np.maximum(std, 1e-12)
    return np.sqrt(np.mean(z * z, axis=0))


def _logvar_head(fn):
    """DenseTrainer's `logvar_head` of a (member) model: (W_v, b_v, min_logvar, max_logvar), None for a plain model."""
    if not hasattr(fn, "logvar_weights"):
        return None
    return fn.logvar_weights, fn.logvar_bias, fn.min_logvar, fn.max_logvar


class SystemDynamicsHandler:
    def __init__(self, env_action_space, env_observation_space, dynamics_function=None, true_model=False,
                 is_normalized=True, log_dir=None, tf_writer=None, save_model_frequency=1, saved_model_dir=None,
                 transform_targets_func=None, inverse_transform_targets_func=None):
        # custom target transforms (reference :128-161 applies inverse_transform_targets_func(states, dev), :314
        # transform_targets_func(states, next_states)).  The inverse one runs in torch on the torch-callable path
        # (utils/device_functions.py) and is inlined into the kernels of DeterministicMLP / HipDynamicsFunction when it is a
        # HipInverseTargetTransform (trajectory_evaluators/deterministic.py); train() applies the forward one per episode
        self._transform_targets_func = transform_targets_func
        self._inverse_transform_targets_func = inverse_transform_targets_func
        self._is_true_model = bool(true_model)
        self._dim_S = int(env_observation_space.shape[0])
        self._dim_U = int(env_action_space.shape[0])
        self._env_action_space = env_action_space
        self._env_observation_space = env_observation_space
        self._dynamics_function = dynamics_function
        self._is_normalized = bool(is_normalized)
        self._log_dir, self._tf_writer = log_dir, tf_writer
        self._save_model_frequency, self._saved_model_dir = save_model_frequency, saved_model_dir
        self._stats = None
        self._version = 0
        # training state (:50-56)
        self._model_training_in = np.zeros((0, self._dim_U + self._dim_S), np.float32)
        self._model_validation_in = np.zeros((0, self._dim_U + self._dim_S), np.float32)
        self._model_training_out = np.zeros((0, self._dim_S), np.float32)
        self._model_validation_out = np.zeros((0, self._dim_S), np.float32)
        self._training_iter = 0
        self._refining_model_iter = 0
        self._first_time = True
        self.training_loss = None
        self.validation_loss = None
        self.multistep_rmse = None                       # (rmse [horizon, S], windows) of the last multistep_error call, on
                                                         # whatever episodes it was given (the learning loops: the ones just trained on)
        if saved_model_dir is not None:
            self.load(saved_model_dir)
            self._first_time = False                     # :61 a loaded model keeps its statistics

    # -- normalisation statistics (system_dynamics_handler.py:84-95, 340-349) -----------------------
    def set_normalization_stats(self, mean_states, std_states, mean_actions, std_actions, mean_targets, std_targets):
        vals = [np.asarray(v, np.float32).reshape(-1) for v in
                (mean_states, std_states, mean_actions, std_actions, mean_targets, std_targets)]
        want = [self._dim_S, self._dim_S, self._dim_U, self._dim_U, self._dim_S, self._dim_S]
        for v, w, n in zip(vals, want, _STATS):
            if v.shape[0] != w:
                raise ValueError("%s must have %d entries" % (n, w))
        self._stats = vals
        self._version += 1

    def normalization_stats(self):
        if self._is_true_model or not self._is_normalized:
            return None
        if self._stats is None:
            raise Exception("dynamics handler is normalised but has no statistics yet "
                            "(set_normalization_stats / load)")
        return self._stats

    # -- process_input / process_output (system_dynamics_handler.py:97-161) as stand-alone calls: inside rollouts the same
    # arithmetic is fused into the kernels; called directly they run the device code through the C ABI
    def _io_engine(self):
        eng = self.__dict__.get("_io_eng")
        if eng is None:
            from .. import _lib as L
            from ..engine import Engine
            eng = self._io_eng = Engine(L.OPT_NONE, L.DYN_USER, L.REW_USER, self._env_action_space.low,
                                        self._env_action_space.high, dim_s=self._dim_S, num_agents=1, planning_horizon=1)
        return eng

    def process_input(self, states, actions):
        """states [B,S], actions [B,U] -> [B,S+U]: concat (true / un-normalised model) or z-scored concat."""
        return self._io_engine().process_input(states, actions, self.normalization_stats())

    def process_output(self, inputs_states, raw_output):
        """inputs_states [B,S], raw_output [B,S] -> absolute next states (de-normalise, then state + delta)."""
        return self._io_engine().process_output(inputs_states, raw_output, self.normalization_stats())

    def load(self, saved_model_dir):
        """Counterpart of the reference's checkpoint load (:78-95): the six `.npy` statistics are read as
        written by the reference; the SavedModel graph is replaced by `mlp.npz` (DeterministicMLP.save)."""
        from ..dynamics_functions.deterministic_mlp import DeterministicMLP
        mlp = os.path.join(saved_model_dir, "mlp.npz")
        if os.path.exists(mlp):
            if os.path.exists(os.path.join(saved_model_dir, "mlp_member1.npz")):      # EnsembleMLP.save
                from ..dynamics_functions.ensemble_mlp import EnsembleMLP
                self._dynamics_function = EnsembleMLP.load(mlp)
            elif os.path.exists(os.path.join(saved_model_dir, "mlp_logvar.npz")):   # ProbabilisticMLP.save
                from ..dynamics_functions.probabilistic_mlp import ProbabilisticMLP
                self._dynamics_function = ProbabilisticMLP.load(mlp)
            else:
                self._dynamics_function = DeterministicMLP.load(mlp)
        if self._is_normalized and all(os.path.exists(os.path.join(saved_model_dir, n + ".npy")) for n in _STATS):
            self.set_normalization_stats(*[np.load(os.path.join(saved_model_dir, n + ".npy")) for n in _STATS])

    def save(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        if hasattr(self._dynamics_function, "save"):
            self._dynamics_function.save(os.path.join(log_dir, "mlp.npz"))
            stale = os.path.join(log_dir, "mlp_logvar.npz")                # a probabilistic model saved here before
            if not getattr(self._dynamics_function, "logvar_heads", None) and os.path.exists(stale):
                os.remove(stale)
        if self._stats is not None:
            for n, v in zip(_STATS, self._stats):
                np.save(os.path.join(log_dir, n + ".npy"), v)

    # -- training (system_dynamics_handler.py:163-349) ---------------------------------------------------------------
    def _append_to_training_dataset(self, observations_trajectories, actions_trajectories, rewards_trajectories,
                                    validation_split=0.2, split_mask=None):
        """:292-331.  Episodes: observations [T+1, A, S], actions [T, A, U]; rows are (s_t, a_t) -> s_{t+1} - s_t,
        episode-major, then agent, then t.  Each row goes to the training set with probability 1 - validation_split
        (np.random.choice, :311-313); `split_mask` injects that draw (True = training row).  With a transform_targets_func
        the targets are transform(states[T,S], next_states[T,S]) per episode and agent (:314)."""
        acs_all = np.array(actions_trajectories)
        num_agents = acs_all.shape[2]
        d_in, d_out = [], []
        for obs, acs in zip(observations_trajectories, acs_all):
            obs = np.asarray(obs)
            for agent in range(num_agents):
                states = obs[:-1, agent]
                d_in.append(np.concatenate([states, acs[:, agent]], axis=-1))
                if self._transform_targets_func is None:
                    d_out.append(obs[1:, agent] - states)                  # default_transform_targets
                else:
                    d_out.append(self._transform_targets(states, obs[1:, agent]))
        d_in = np.array(d_in, dtype=np.float32).reshape(-1, self._dim_U + self._dim_S)
        d_out = np.array(d_out, dtype=np.float32).reshape(-1, self._dim_S)
        if split_mask is None:
            split_mask = np.random.choice([False, True], size=d_in.shape[0], p=[validation_split, 1.0 - validation_split])
        split_mask = np.asarray(split_mask, bool)
        if split_mask.shape[0] != d_in.shape[0]:
            raise ValueError("split_mask needs one entry per transition (%d)" % d_in.shape[0])
        self._model_training_in = np.concatenate([self._model_training_in, d_in[split_mask]], axis=0)
        self._model_training_out = np.concatenate([self._model_training_out, d_out[split_mask]], axis=0)
        self._model_validation_in = np.concatenate([self._model_validation_in, d_in[~split_mask]], axis=0)
        self._model_validation_out = np.concatenate([self._model_validation_out, d_out[~split_mask]], axis=0)

    def _transform_targets(self, states, next_states):
        """transform_targets_func(states[T,S], next_states[T,S]) -> [T,S] on float32 arrays: any NumPy callable, or a
        HipTargetTransform (run on the GPU)."""
        s = np.ascontiguousarray(states, np.float32)
        n = np.ascontiguousarray(next_states, np.float32)
        out = np.asarray(self._transform_targets_func(s, n), np.float32)
        if out.shape != s.shape:
            raise ValueError("transform_targets_func returned shape %s for states of shape %s" % (out.shape, s.shape))
        return out

    def _recompute_normalization(self):
        """:340-349 -- statistics of the TRAINING rows (population std)."""
        S = self._dim_S
        tin, tout = self._model_training_in, self._model_training_out
        self.set_normalization_stats(np.mean(tin[:, :S], axis=0), np.std(tin[:, :S], axis=0),
                                     np.mean(tin[:, S:], axis=0), np.std(tin[:, S:], axis=0),
                                     np.mean(tout, axis=0), np.std(tout, axis=0))

    def _normalize_data(self, data_in, data_out):
        """:333-338; un-normalised handlers train on the raw rows."""
        if not self._is_normalized:
            return data_in, data_out
        ms, ss, ma, sa, mt, st = self._stats
        S = self._dim_S
        s = (data_in[:, :S] - ms) / (ss + 1e-7)
        a = (data_in[:, S:] - ma) / (sa + 1e-7)
        t = (data_out - mt) / (st + 1e-7)
        return np.concatenate([s, a], axis=1).astype(np.float32), t.astype(np.float32)

    def train(self, observations_trajectories, actions_trajectories, rewards_trajectories, validation_split=0.2,
              batch_size=128, learning_rate=1e-3, epochs=30, nn_optimizer=None, *, device=None, seed=None,
              split_mask=None, permutations=None, bootstrap_indices=None, backend="torch", weight_decay=0.0, decay_mode="l2",
              patience=0, min_delta=0.0, restore_best=False):
        """Reference signature (:163-166); `nn_optimizer`: None / "Adam" / "SGD" / "RMSprop" or a class of that name
        (the reference's callers only ever pass tf.keras.optimizers.Adam).  Keyword-only extras: `device` (default: the GPU -- training on the
        host has to be asked for explicitly with device="cpu"), and the injected random draws `split_mask`,
        `permutations` (one per epoch) / `seed` for reproducible runs.  With an EnsembleMLP every member is fitted on
        its own bootstrap resample of the training rows (`_train_ensemble`; `bootstrap_indices` injects the resamples).
        A ProbabilisticMLP (or an ensemble of them) is fitted, mean and log-variance head together, on the Gaussian
        negative log-likelihood: training_loss / validation_loss (and the member lists) then hold the NLL, while
        residual_std() stays the mean network's residual.  `backend`: "torch" (DenseTrainer, the default) or "hip"
        (dynamics_functions/_train_hip.HipDenseTrainer: the hand-written training kernels, GPU only, plain MSE models --
        a model with a log-variance head is refused by name; the members of an EnsembleMLP are fitted by one
        HipEnsembleTrainer, all of them in one launch sequence) or "hip_nll" ("hip" for a model without a log-variance head,
        the same trainers and bits; a ProbabilisticMLP is fitted by a HipGaussianTrainer and the members of an
        EnsembleMLP(probabilistic=True) by ONE HipGaussianEnsembleTrainer: the Gaussian NLL in the same kernels, DESIGN.md
        section 8s).
        `weight_decay` (a scalar or one value per layer, kernels only) / `decay_mode` ("l2" | "decoupled"), `patience` /
        `min_delta` (early stopping on the validation loss) and `restore_best` (the best epoch's weights are installed):
        dynamics_functions/_train_reg.py; both backends, every member of an ensemble on its own.
        They reach the trainer only where they differ from the defaults.  `epochs_run` / `best_epoch` (and
        `member_epochs_run` / `member_best_epoch`) record the fit; residual_std() is that of the installed weights."""
        from ..dynamics_functions._train_hip import check_backend, dense_trainer
        from ..dynamics_functions._train_reg import non_default
        check_backend(backend)
        reg = non_default(weight_decay, decay_mode, patience, min_delta, restore_best)
        if self._is_true_model:
            raise Exception("the true model has nothing to train")
        # the reference instantiates `nn_optimizer(learning_rate=learning_rate)` (:261): a Keras optimizer CLASS (or its
        # name); Adam / SGD / RMSprop with their TF-2.0 defaults are built
        rule = "adam" if nn_optimizer is None else getattr(nn_optimizer, "__name__", str(nn_optimizer)).lower()
        if rule not in ("adam", "sgd", "rmsprop"):
            raise NotImplementedError("nn_optimizer %r: Adam, SGD and RMSprop (Keras defaults) are built" % (nn_optimizer,))
        fn = self._dynamics_function
        if fn is None or not hasattr(fn, "weights"):
            raise Exception("train() needs a DeterministicMLP dynamics function")
        if backend == "hip" and getattr(fn, "logvar_heads", None):
            raise ValueError("backend='hip' fits plain Dense stacks (MSE): %s has a log-variance head (Gaussian NLL) and "
                             "trains with backend='torch' or backend='hip_nll'" % type(fn).__name__)
        if device is None and backend == "torch":
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("SystemDynamicsHandler.train runs on the GPU and none is visible "
                                   "(pass device='cpu' explicitly to train on the host)")
            device = "cuda"
        self._append_to_training_dataset(observations_trajectories, actions_trajectories, rewards_trajectories,
                                         validation_split=validation_split, split_mask=split_mask)
        if self._first_time:                                               # :193-198 statistics are frozen after the first call
            if self._is_normalized:
                self._recompute_normalization()
            self._first_time = False
        tin, tout = self._normalize_data(self._model_training_in, self._model_training_out)
        vin, vout = self._normalize_data(self._model_validation_in, self._model_validation_out)
        if hasattr(fn, "members"):
            self._train_ensemble(fn, tin, tout, vin, vout, epochs, batch_size, learning_rate, rule, device, seed, permutations,
                                 bootstrap_indices, backend, reg)
            return self._after_training()
        if bootstrap_indices is not None:
            raise ValueError("bootstrap_indices are the resamples of an EnsembleMLP's members")
        trainer = dense_trainer(backend, fn.weights, fn.biases, fn.activation_codes, device, learning_rate=learning_rate, rule=rule,
                                logvar_head=_logvar_head(fn), **reg)       # fresh optimizer per call (:258)
        self.training_loss, self.validation_loss = trainer.fit(tin, tout, vin, vout, epochs, batch_size,
                                                               permutations=permutations, generator_seed=seed)
        self.epochs_run, self.best_epoch = getattr(trainer, "epochs_run", epochs), getattr(trainer, "best_epoch", -1)
        self._residual_rms = trainer.residual_rms(vin, vout)              # normalised target units; residual_std() scales it
        self._trained = True
        fn.set_weights(*trainer.numpy_params())                            # bumps the version: evaluators re-upload
        if trainer.has_logvar_head:
            fn.set_logvar_head(*trainer.numpy_logvar_head())
        return self._after_training()

    def _after_training(self):
        self._version += 1
        self._refining_model_iter += 1                                     # :290
        self._training_iter += 1
        if self._training_iter % self._save_model_frequency == 0 and self._log_dir is not None:   # :212-241
            self.save(os.path.join(self._log_dir, "saved_model_%d" % self._refining_model_iter))
        return

    def _train_ensemble(self, fn, tin, tout, vin, vout, epochs, batch_size, learning_rate, rule, device, seed, permutations,
                        bootstrap_indices, backend="torch", reg=None):
        """The members of an EnsembleMLP on the (normalised) rows train() prepared -- statistics, split and the
        freeze-after-first rule are shared.  Member e is fitted by a fresh trainer (backend "hip": all members by one
        HipEnsembleTrainer, `_fit_members_hip`, with the same results) on a bootstrap resample of the training rows: n_train indices drawn with replacement, `bootstrap_indices[e]` when given, else from
        np.random.default_rng([seed, e]) -- which then also draws the member's epoch permutations.  Injected
        `permutations` are [E][epochs] (one list per member) or [epochs] (shared by the members).
        training_loss / validation_loss stay member 0's; the per-member lists go to member_training_loss /
        member_validation_loss, and residual_std() becomes the RMS over members of the members' validation residuals.
        `reg`: train()'s non-default regularisation options, for every member's trainer; member_epochs_run /
        member_best_epoch record each member's fit, epochs_run / best_epoch member 0's."""
        from ..dynamics_functions._train_hip import dense_trainer
        reg = dict(reg or {})
        n, members = tin.shape[0], fn.members
        if bootstrap_indices is not None:
            if len(bootstrap_indices) != len(members):
                raise ValueError("bootstrap_indices needs one row of indices per member (%d)" % len(members))
            bootstrap_indices = [np.asarray(ix, np.int64).reshape(-1) for ix in bootstrap_indices]
            for ix in bootstrap_indices:
                if ix.shape[0] != n or (n and (ix.min() < 0 or ix.max() >= n)):
                    raise ValueError("bootstrap_indices: %d indices into the %d training rows per member" % (n, n))
        per_member = permutations is not None and len(permutations) > 0 and np.ndim(permutations[0]) >= 2
        if per_member and len(permutations) != len(members):
            raise ValueError("permutations needs one list per member (%d)" % len(members))
        draws = []                                                          # per member: (bootstrap rows, epoch permutations)
        for e in range(len(members)):
            rng = np.random.default_rng([int(seed), e] if seed is not None else None)
            idx = bootstrap_indices[e] if bootstrap_indices is not None else rng.integers(0, n, size=n)
            if permutations is None:
                perms = [rng.permutation(n) for _ in range(epochs)]
            else:
                perms = permutations[e] if per_member else permutations
            draws.append((idx, perms))
        if backend in ("hip", "hip_nll"):                                  # (train() refused "hip" on a probabilistic ensemble)
            tl, vl, rms, ran, best = self._fit_members_hip(members, draws, tin, tout, vin, vout, epochs, batch_size, learning_rate, rule,
                                                           device, seed, reg)
        else:
            tl, vl, rms, ran, best = [], [], [], [], []
            for member, (idx, perms) in zip(members, draws):
                trainer = dense_trainer(backend, member.weights, member.biases, member.activation_codes, device,
                                        learning_rate=learning_rate, rule=rule, logvar_head=_logvar_head(member), **reg)
                tl_e, vl_e = trainer.fit(tin[idx], tout[idx], vin, vout, epochs, batch_size, permutations=perms, generator_seed=seed)
                tl.append(tl_e)
                vl.append(vl_e)
                ran.append(getattr(trainer, "epochs_run", epochs))
                best.append(getattr(trainer, "best_epoch", -1))
                rms.append(trainer.residual_rms(vin, vout))
                member.set_weights(*trainer.numpy_params())                # bumps the version: evaluators re-upload
                if trainer.has_logvar_head:
                    member.set_logvar_head(*trainer.numpy_logvar_head())
        self.member_training_loss, self.member_validation_loss = tl, vl
        self.training_loss, self.validation_loss = self.member_training_loss[0], self.member_validation_loss[0]
        self.member_epochs_run, self.member_best_epoch = [int(v) for v in ran], [int(v) for v in best]
        self.epochs_run, self.best_epoch = self.member_epochs_run[0], self.member_best_epoch[0]
        self._residual_rms = None if rms[0] is None else np.sqrt(np.mean(np.square(np.asarray(rms, np.float64)), axis=0)).astype(np.float32)
        self._trained = True

    @staticmethod
    def _fit_members_hip(members, draws, tin, tout, vin, vout, epochs, batch_size, learning_rate, rule, device, seed, reg=None):
        """`_train_ensemble`'s loop as ONE HipEnsembleTrainer and one fit ("Members"): the rows go to
        the device once, member e's bootstrap resample is the index map `member_rows[e]`, and every step is one launch pair
        for all members.  Bit for bit what a HipDenseTrainer per member on `tin[idx]` gives.  Returns the per-member lists
        (training loss, validation loss, residual RMS -- of the weights the fit leaves, restored ones included -- epochs run,
        best epoch).  Members with a log-variance head (backend "hip_nll" on a probabilistic ensemble) are fitted the same way
        by ONE HipGaussianEnsembleTrainer: the losses are then the NLL, the residual stays the mean network's, and the heads
        are installed with the weights."""
        from ..dynamics_functions import _train_hip as T
        if _logvar_head(members[0]) is None:
            trainer = T.HipEnsembleTrainer([m.weights for m in members], [m.biases for m in members], members[0].activation_codes,
                                           device, learning_rate=learning_rate, rule=rule, **(reg or {}))
        else:
            trainer = T.HipGaussianEnsembleTrainer(
                [m.weights for m in members], [m.biases for m in members], members[0].activation_codes, device,
                learning_rate=learning_rate, rule=rule, logvar_heads=[(m.logvar_weights, m.logvar_bias) for m in members],
                min_logvar=members[0].min_logvar, max_logvar=members[0].max_logvar, **(reg or {}))
        try:
            tl, vl = trainer.fit(tin, tout, vin, vout, epochs, batch_size, member_rows=[idx for idx, _ in draws],
                                 permutations=[np.asarray(perms)[:epochs] for _, perms in draws], generator_seed=seed)
            rms = trainer.residual_rms(vin, vout)
            for e, member in enumerate(members):
                member.set_weights(*trainer.numpy_params(e))               # bumps the version: evaluators re-upload
                if getattr(trainer, "has_logvar_head", False):
                    member.set_logvar_head(*trainer.numpy_logvar_head(e))
        finally:
            trainer.close()
        ran = getattr(trainer, "epochs_run", [epochs] * len(members))
        best = getattr(trainer, "best_epoch", [-1] * len(members))
        return list(tl), list(vl), ([None] * len(members) if rms is None else list(rms)), list(ran), list(best)

    def residual_std(self):
        """Per-dimension RMS of (target - prediction) in state units on the held-out validation rows of the last train():
        the one-step residual of the fitted model, the natural `process_noise_std` of a ParticleTrajectoryEvaluator.
        Computed by train() on the device it trains on."""
        if not getattr(self, "_trained", False):
            raise Exception("residual_std() needs a train() call first")
        if self._residual_rms is None:
            raise Exception("residual_std(): the last train() held no validation rows out (validation_split / split_mask)")
        r = np.asarray(self._residual_rms, np.float32)
        if self._is_normalized:
            r = r * (np.asarray(self._stats[5], np.float32) + np.float32(1e-7))     # targets were (t - mean_t) / (std_t + 1e-7)
        return r.astype(np.float32)

    # -- multi-step (open-loop) model error ---------------------------------------------------------------------------
    def _multistep_engine(self):
        """An evaluator-only engine of this handler's model, one per GPU, for states-only trajectory prediction.  A handle
        has to be created with some reward kind: the pendulum's where dim_S allows it, else BBMPC_REW_USER without a
        source.  Neither is ever evaluated -- multistep_error passes rewards_out = NULL, and for that the engine rolls a
        learned model through its MFMA trajectory kernel whatever the reward kind is (bbmpc_traj.hip)."""
        from .. import _lib as L
        from ..engine import Engine
        from ..trajectory_evaluators import deterministic as D
        import torch
        engines = self.__dict__.setdefault("_ms_engines", {})
        device = torch.cuda.current_device()
        eng = engines.get(device)
        if eng is None:
            dyn = D.dynamics_plugin(self)
            dk = getattr(dyn, "_bbmpc_dynamics_kind", None)
            eng = engines[device] = Engine(L.OPT_NONE, L.DYN_USER if dk is None else dk,
                                           L.REW_PENDULUM if self._dim_S >= 3 else L.REW_USER, self._env_action_space.low,
                                           self._env_action_space.high, dim_s=self._dim_S, num_agents=1, planning_horizon=1,
                                           device=device)
        if D.dynamics_stale(eng, self):
            D.configure_dynamics(eng, self)
        if eng._param_fns:
            from ..utils.device_functions import sync_user_params
            sync_user_params(eng)
        return eng

    def multistep_error(self, observations_trajectories, actions_trajectories, horizon, stride=1, max_rows=262144):
        """Open-loop error of the model over `horizon` steps on episodes in train()'s layout: every window
        (multistep_windows) is rolled out from its first observation under the recorded actions on the GPU
        (bbmpc_predict_trajectories_dev) and compared with the recorded states there (bbmpc_trajectory_sq_error_dev, a
        deterministic reduction).  Returns (rmse [horizon, dim_S] in state units, number of windows) and keeps it in
        `multistep_rmse`.  A true model on its own data gives ~0."""
        import torch
        starts, acts, observed = multistep_windows(observations_trajectories, actions_trajectories, horizon, stride)
        n, horizon = starts.shape[0], int(horizon)
        if n == 0:
            raise ValueError("multistep_error: no episode is %d steps long" % horizon)
        if starts.shape[1] != self._dim_S or acts.shape[2] != self._dim_U:
            raise ValueError("multistep_error: episodes of dim_S %d / dim_U %d for a handler of %d / %d"
                             % (starts.shape[1], acts.shape[2], self._dim_S, self._dim_U))
        eng = self._multistep_engine()
        dev = torch.device("cuda", eng.device)
        total = np.zeros(horizon * self._dim_S, np.float64)
        for r0 in range(0, n, int(max_rows)):
            r1 = min(n, r0 + int(max_rows))
            d_s = torch.from_numpy(starts[r0:r1]).to(dev)
            d_a = torch.from_numpy(acts[r0:r1]).to(dev)
            d_o = torch.from_numpy(observed[r0:r1]).to(dev)
            d_p = torch.empty_like(d_o)
            d_e = torch.empty(horizon * self._dim_S, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)                                    # the copies above ran on torch's stream
            eng.predict_trajectories_dev(d_s.data_ptr(), d_a.data_ptr(), r1 - r0, horizon, d_p.data_ptr(), 0)
            eng.trajectory_sq_error_dev(d_p.data_ptr(), d_o.data_ptr(), r1 - r0, horizon, d_e.data_ptr())
            eng.synchronize()
            total += d_e.cpu().numpy()
        rmse = np.sqrt(total / n).reshape(horizon, self._dim_S)
        self.multistep_rmse = (rmse, n)
        return rmse, n

    def multistep_calibration(self, observations_trajectories, actions_trajectories, horizon, stride, evaluator):
        """Is the spread a ParticleTrajectoryEvaluator predicts honest?  Every window of `horizon` steps
        (multistep_windows) is rolled out from its first observation under the recorded actions as a particle distribution
        (evaluator.predict_trajectory_distribution) and the recorded states are standardised against it.  Returns
        (z_rms [horizon, dim_S] -- calibration_z_rms, about 1 for an honest spread -- and the number of windows) and keeps
        it in `multistep_z_rms`."""
        if not hasattr(evaluator, "predict_trajectory_distribution"):
            raise TypeError("multistep_calibration() needs a ParticleTrajectoryEvaluator, got %s" % type(evaluator).__name__)
        starts, acts, observed = multistep_windows(observations_trajectories, actions_trajectories, horizon, stride)
        n = starts.shape[0]
        if n == 0:
            raise ValueError("multistep_calibration: no episode is %d steps long" % int(horizon))
        if starts.shape[1] != self._dim_S or acts.shape[2] != self._dim_U:
            raise ValueError("multistep_calibration: episodes of dim_S %d / dim_U %d for a handler of %d / %d"
                             % (starts.shape[1], acts.shape[2], self._dim_S, self._dim_U))
        mean, std = evaluator.predict_trajectory_distribution(starts, acts)[:2]
        z_rms = calibration_z_rms(mean, std, observed)
        self.multistep_z_rms = (z_rms, n)
        return z_rms, n
