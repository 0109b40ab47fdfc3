"""LearnedPolicyMLP -- a policy network pi(s) whose closed-loop rollouts through the learned model join CEM's candidates
(the policy prior of TD-MPC, POLO and LOOP-style planners).

A weights container like LearnedValueMLP: Dense kernels [in, out] + biases, Keras default init, the state as input, one
output per action dimension.  At planning time the network alternates with the dynamics network on the matrix cores
(bbmpc_set_policy_prior_mlp; csrc/kernels_policy_prior.hpp, k_policy_prior_rollout); `train` fits it by regression on
(state, action) pairs -- behaviour cloning of the actions MPC executed -- with dynamics_functions/_train_torch.py.
`__call__(states)` evaluates it on NumPy arrays."""
import numpy as np

from ..dynamics_functions.deterministic_mlp import _ACT_NAME, _act_code
from ..reward_functions.learned_reward_mlp import numpy_activation


class LearnedPolicyMLP:
    def __init__(self, dim_S, dim_U, layers, activations, seed=None, name=None):
        """layers: the Dense widths behind the state, ending in dim_U (e.g. [200, 200, dim_U]); activations: one per Dense
        layer (names or callables, as DeterministicMLP takes them)."""
        self.name = name
        self.dim_S, self.dim_U = int(dim_S), int(dim_U)
        widths = [int(v) for v in layers]
        if not widths or widths[-1] != self.dim_U:
            raise ValueError("a policy network ends in dim_U = %d outputs: layers[-1] is %r" % (self.dim_U, layers))
        if len(activations) != len(widths):
            raise ValueError("need one activation per Dense layer")
        self.layer_sizes = [self.dim_S] + widths
        self.activation_codes = [_act_code(a) for a in activations]
        rng = np.random.default_rng(seed)
        self.weights, self.biases = [], []
        for i in range(1, len(self.layer_sizes)):
            fan_in, fan_out = self.layer_sizes[i - 1], self.layer_sizes[i]
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            self.weights.append(rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32))
            self.biases.append(np.zeros((fan_out,), np.float32))
        self._stats = None                  # (mean_in [S], std_in [S], mean_out [U], std_out [U]) once trained / set
        self._version = 0
        self._pairs = []                    # (states, actions) collected by train_on_rollouts

    # -- parameters ---------------------------------------------------------------------------------------------------
    def set_weights(self, weights, biases):
        if len(weights) != len(self.weights):
            raise ValueError("expected %d layers" % len(self.weights))
        for i, (w, b) in enumerate(zip(weights, biases)):
            w = np.asarray(w, np.float32)
            b = np.asarray(b, np.float32).reshape(-1)
            if w.shape != self.weights[i].shape or b.shape != self.biases[i].shape:
                raise ValueError("layer %d shape mismatch" % i)
            self.weights[i], self.biases[i] = w.copy(), b.copy()
        self._version += 1

    def set_normalization_stats(self, stats):
        """stats = (mean_in [S], std_in [S], mean_out [U], std_out [U]) or None (an un-normalised network)."""
        if stats is None:
            self._stats = None
        else:
            mi, si, mo, so = [np.asarray(s, np.float32).reshape(-1) for s in stats]
            if mi.shape != (self.dim_S,) or si.shape != (self.dim_S,) or mo.shape != (self.dim_U,) or so.shape != (self.dim_U,):
                raise ValueError("stats must be (mean_in [%d], std_in [%d], mean_out [%d], std_out [%d])"
                                 % (self.dim_S, self.dim_S, self.dim_U, self.dim_U))
            self._stats = (mi.copy(), si.copy(), mo.copy(), so.copy())
        self._version += 1

    def normalization_stats(self):
        return self._stats

    # -- evaluation on the host -----------------------------------------------------------------------------------------
    def __call__(self, states):
        """pi(states [B, S]) -> [B, U] float32, computed in float64 on the host: normalise as
        SystemDynamicsHandler.process_input does, the Dense stack, y * std_out + mean_out.  No noise, no clip."""
        x = np.asarray(states).reshape(-1, self.dim_S).astype(np.float64)
        if self._stats is not None:
            x = (x - self._stats[0].astype(np.float64)) / (self._stats[1].astype(np.float64) + np.float64(np.float32(1e-7)))
        for w, b, a in zip(self.weights, self.biases, self.activation_codes):
            x = numpy_activation(a, x @ w.astype(np.float64) + b.astype(np.float64))
        if self._stats is not None:
            x = x * self._stats[3].astype(np.float64) + self._stats[2].astype(np.float64)
        return x.astype(np.float32)

    # -- training -------------------------------------------------------------------------------------------------------
    def train(self, states, actions, epochs=30, batch_size=128, learning_rate=1e-3, validation_split=0.2, device=None,
              seed=None, normalize=True, backend="torch", *, weight_decay=0.0, decay_mode="l2",
              patience=0, min_delta=0.0, restore_best=False):
        """Fit MSE on normalised targets with Keras-Adam (dynamics_functions/_train_torch.DenseTrainer, on `device`: the
        GPU when PyTorch sees one, else the CPU).  states [B, S], actions [B, U].  The statistics are refreshed from exactly
        these rows and the version is bumped, so every engine that holds the network uploads it again before its next
        computation.  Returns (train_loss [epochs], validation_loss [epochs]).
        backend: "torch" (the default), "hip" or "hip_nll" (here the same as "hip") -- the hand-written training kernels
        (dynamics_functions/_train_hip.HipDenseTrainer; GPU only, permutations drawn by the library from `seed`).
        weight_decay / decay_mode / patience / min_delta / restore_best (keyword-only): weight decay on the kernels, early
        stopping on the validation loss and best-weights restore (dynamics_functions/_train_reg.py),
        handed to the trainer only where they differ from the defaults; `epochs_run` / `best_epoch` record the fit."""
        from ..dynamics_functions._train_hip import check_backend, dense_trainer
        from ..dynamics_functions._train_reg import non_default
        check_backend(backend)
        reg = non_default(weight_decay, decay_mode, patience, min_delta, restore_best)
        x = np.asarray(states, np.float32).reshape(-1, self.dim_S)
        y = np.asarray(actions, np.float32).reshape(-1, self.dim_U)
        if x.shape[0] != y.shape[0]:
            raise ValueError("%d state rows but %d action rows" % (x.shape[0], y.shape[0]))
        if normalize:
            stats = [np.asarray(s, np.float32) for s in (x.mean(axis=0), x.std(axis=0), y.mean(axis=0), y.std(axis=0))]
            stats[3] = np.where(stats[3] > 0, stats[3], np.float32(1.0)).astype(np.float32)      # constant targets stay centred
            stats = tuple(stats)
            xn = (x - stats[0]) / (stats[1] + np.float32(1e-7))
            yn = (y - stats[2]) / stats[3]
        else:
            stats, xn, yn = None, x, y
        rng = np.random.default_rng(seed)
        order = rng.permutation(x.shape[0])
        n_val = int(x.shape[0] * float(validation_split))
        val, trn = order[:n_val], order[n_val:]
        if device is None and backend == "torch":
            import torch
            device = "cuda" if torch.cuda.is_available() else "cpu"
        tr = dense_trainer(backend, self.weights, self.biases, self.activation_codes, device, learning_rate=learning_rate, **reg)
        bs = max(1, min(int(batch_size), len(trn)))
        losses = tr.fit(xn[trn], yn[trn], xn[val], yn[val], int(epochs), bs,
                        generator_seed=None if seed is None else int(seed))
        ws, bs_ = tr.numpy_params()
        self._stats = stats
        self.set_weights(ws, bs_)
        self.train_loss, self.validation_loss = [float(v) for v in losses[0]], [float(v) for v in losses[1]]
        self.epochs_run, self.best_epoch = getattr(tr, "epochs_run", int(epochs)), getattr(tr, "best_epoch", -1)
        return losses

    def train_on_rollouts(self, traj_obs, traj_acs, **train_args):
        """Add the episodes perform_rollouts returned (observations [T+1,A,S], executed actions [T,A,U] each) to those
        collected so far and refit on all (observation, action) pairs."""
        for obs, acs in zip(traj_obs, traj_acs):
            obs, acs = np.asarray(obs, np.float32), np.asarray(acs, np.float32)
            T = acs.shape[0]
            self._pairs.append((obs[:T].reshape(-1, self.dim_S), acs.reshape(-1, self.dim_U)))
        states = np.concatenate([p[0] for p in self._pairs], axis=0)
        actions = np.concatenate([p[1] for p in self._pairs], axis=0)
        return self.train(states, actions, **train_args)

    # -- persistence ----------------------------------------------------------------------------------------------------
    def save(self, path):
        extra = {}
        if self._stats is not None:
            extra = {"mean_in": self._stats[0], "std_in": self._stats[1], "mean_out": self._stats[2], "std_out": self._stats[3]}
        np.savez(path, dim_S=self.dim_S, dim_U=self.dim_U, n_layers=len(self.weights), layers=np.array(self.layer_sizes[1:]),
                 activations=np.array(self.activation_codes),
                 **{"W%d" % i: w for i, w in enumerate(self.weights)}, **{"b%d" % i: b for i, b in enumerate(self.biases)}, **extra)

    @classmethod
    def load(cls, path):
        z = np.load(path)
        m = cls(int(z["dim_S"]), int(z["dim_U"]), list(z["layers"]), [_ACT_NAME[int(c)] for c in z["activations"]])
        n = int(z["n_layers"])
        m.set_weights([z["W%d" % i] for i in range(n)], [z["b%d" % i] for i in range(n)])
        if "mean_in" in z.files:
            m.set_normalization_stats((z["mean_in"], z["std_in"], z["mean_out"], z["std_out"]))
        return m
