"""LearnedValueMLP -- a value network V(s) that closes a short planning horizon: R = sum_t r_t + w * V(s_H), the terminal
term of POLO, TD-MPC and MBPO-style planners.

A weights container like LearnedRewardMLP: Dense kernels [in, out] + biases, Keras default init, one output, the state
alone as input.  At planning time the network runs on the matrix cores over the last state of every learned-model rollout
(bbmpc_set_terminal_value_mlp; csrc/kernels_reward_mlp.hpp, k_value_mlp_terminal); `train` fits it with
dynamics_functions/_train_torch.py.  `__call__(states)` evaluates it on NumPy arrays."""
import numpy as np

from ..dynamics_functions.deterministic_mlp import _ACT_NAME, _act_code
from ..reward_functions.learned_reward_mlp import numpy_activation


def value_targets(traj_obs, traj_rews, n_step, gamma=1.0, bootstrap=None, terminated=None):
    """n-step return targets of one episode: observations [T+1, A, S], rewards [T, A] -> (states [M, S], targets [M]) with
    M = (T - n_step + 1) * A rows, one per (t, agent) with t <= T - n_step (full windows only; none when n_step > T):
        y_t = sum_{k < n_step} gamma^k r_{t+k}  (+ gamma^n_step * bootstrap(s_{t+n_step}) when `bootstrap` is a callable
    states [B, S] -> [B]).
    terminated: bool [T, A] (or [T] for every agent), true where step t reached a terminal state.  A window then stops at
    its first terminal step -- that step's reward counts, nothing behind it does -- and takes no bootstrap: what the shaped
    returns of the planner do (bbmpc_set_return_shaping).  Rows whose own step lies behind an agent's first terminal step
    are still returned: the caller decides what an episode is.  None reproduces the targets without it."""
    obs = np.asarray(traj_obs, np.float32)
    rews = np.asarray(traj_rews, np.float32)
    n_step = int(n_step)
    if n_step < 1:
        raise ValueError("n_step must be >= 1")
    T = rews.shape[0]
    if obs.ndim != 3 or obs.shape[0] != T + 1:
        raise ValueError("observations [T+1, A, S] and rewards [T, A] expected, got %s and %s" % (obs.shape, rews.shape))
    A, S = obs.shape[1], obs.shape[2]
    rews = rews.reshape(T, A)
    M = T - n_step + 1
    if M <= 0:
        return np.zeros((0, S), np.float32), np.zeros((0,), np.float32)
    y = np.zeros((M, A), np.float64)
    if terminated is None:
        for k in range(n_step):
            y += float(gamma) ** k * rews[k:k + M].astype(np.float64)
        alive = None
    else:
        done = np.asarray(terminated, bool)
        if done.shape not in ((T,), (T, A)):
            raise ValueError("terminated must be [T] or [T, A] = [%d, %d], got %s" % (T, A, done.shape))
        done = np.broadcast_to(done.reshape(T, -1), (T, A))
        alive = np.ones((M, A), bool)                  # the window has not met a terminal step yet
        for k in range(n_step):
            y += np.where(alive, float(gamma) ** k * rews[k:k + M].astype(np.float64), 0.0)
            alive = alive & ~done[k:k + M]
    if bootstrap is not None:
        tail = np.asarray(bootstrap(obs[n_step:n_step + M].reshape(M * A, S)), np.float64).reshape(M, A)
        y += float(gamma) ** n_step * tail if alive is None else np.where(alive, float(gamma) ** n_step * tail, 0.0)
    return obs[:M].reshape(M * A, S).copy(), y.reshape(M * A).astype(np.float32)


class LearnedValueMLP:
    def __init__(self, dim_S, layers, activations, seed=None, name=None):
        """layers: the Dense widths behind the state, ending in 1 (e.g. [200, 200, 1]); activations: one per Dense layer
        (names or callables, as DeterministicMLP takes them)."""
        self.name = name
        self.dim_S = int(dim_S)
        widths = [int(v) for v in layers]
        if not widths or widths[-1] != 1:
            raise ValueError("a value network ends in one output: layers[-1] must be 1, got %r" % (layers,))
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
        self._stats = None                  # (mean_in [S], std_in [S], mean_v [1], std_v [1]) once trained / set
        self._version = 0
        self._episodes = []                 # (observations, rewards) collected by train_on_rollouts

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
        """stats = (mean_in [S], std_in [S], mean_v, std_v) or None (an un-normalised network)."""
        if stats is None:
            self._stats = None
        else:
            mi, si, mv, sv = [np.asarray(s, np.float32).reshape(-1) for s in stats]
            if mi.shape != (self.dim_S,) or si.shape != (self.dim_S,) or mv.shape != (1,) or sv.shape != (1,):
                raise ValueError("stats must be (mean_in [%d], std_in [%d], mean_v [1], std_v [1])" % (self.dim_S, self.dim_S))
            self._stats = (mi.copy(), si.copy(), mv.copy(), sv.copy())
        self._version += 1

    def normalization_stats(self):
        return self._stats

    # -- evaluation on the host -----------------------------------------------------------------------------------------
    def __call__(self, states):
        """V(states [B, S]) -> [B] float32, computed in float64 on the host: normalise as SystemDynamicsHandler.process_input
        does, the Dense stack, y * std_v + mean_v."""
        x = np.asarray(states).reshape(-1, self.dim_S).astype(np.float64)
        if self._stats is not None:
            x = (x - self._stats[0].astype(np.float64)) / (self._stats[1].astype(np.float64) + np.float64(np.float32(1e-7)))
        for w, b, a in zip(self.weights, self.biases, self.activation_codes):
            x = numpy_activation(a, x @ w.astype(np.float64) + b.astype(np.float64))
        y = x[:, 0]
        if self._stats is not None:
            y = y * np.float64(self._stats[3][0]) + np.float64(self._stats[2][0])
        return y.astype(np.float32)

    # -- training -------------------------------------------------------------------------------------------------------
    def train(self, states, targets, epochs=30, batch_size=128, learning_rate=1e-3, validation_split=0.2, device=None,
              seed=None, normalize=True, backend="torch", *, weight_decay=0.0, decay_mode="l2",
              patience=0, min_delta=0.0, restore_best=False):
        """Fit MSE on normalised targets with Keras-Adam (dynamics_functions/_train_torch.DenseTrainer, on `device`: the
        GPU when PyTorch sees one, else the CPU).  states [B, S], targets [B].  The statistics are refreshed from exactly
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
        y = np.asarray(targets, np.float32).reshape(-1, 1)
        if x.shape[0] != y.shape[0]:
            raise ValueError("%d state rows but %d targets" % (x.shape[0], y.shape[0]))
        if normalize:
            stats = tuple(np.asarray(s, np.float32) for s in (x.mean(axis=0), x.std(axis=0), y.mean(axis=0), y.std(axis=0)))
            xn = (x - stats[0]) / (stats[1] + np.float32(1e-7))
            sv = stats[3] if stats[3][0] > 0 else np.ones((1,), np.float32)          # constant targets stay centred
            stats = (stats[0], stats[1], stats[2], sv)
            yn = (y - stats[2]) / sv
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

    def train_on_rollouts(self, traj_obs, traj_rews, n_step, gamma=1.0, bootstrap=False, terminated=None, **train_args):
        """Add the episodes perform_rollouts returned (observations [T+1,A,S], rewards [T,A] each) to those collected so
        far and refit on the n-step targets of all of them.  bootstrap=True closes every window with the model's own
        current prediction, gamma^n_step * V(s_{t+n_step}) (fitted n-step TD); False fits plain n-step returns.
        terminated: one bool [T,A] array per episode (value_targets' argument; e.g. StateBoxTermination(obs[1:])), so that
        V and a planner with the same termination agree on where an episode ends."""
        traj_obs, traj_rews = list(traj_obs), list(traj_rews)
        dones = [None] * len(traj_obs) if terminated is None else list(terminated)
        if len(dones) != len(traj_obs):
            raise ValueError("terminated: one array per episode expected, got %d for %d episodes" % (len(dones), len(traj_obs)))
        for obs, rews, done in zip(traj_obs, traj_rews, dones):
            self._episodes.append((np.asarray(obs, np.float32), np.asarray(rews, np.float32)) if done is None else
                                  (np.asarray(obs, np.float32), np.asarray(rews, np.float32), np.asarray(done, bool)))
        boot = self.__call__ if bootstrap else None
        rows = [value_targets(e[0], e[1], n_step, gamma, boot, e[2] if len(e) > 2 else None) for e in self._episodes]
        states = np.concatenate([r[0] for r in rows], axis=0)
        targets = np.concatenate([r[1] for r in rows], axis=0)
        if states.shape[0] == 0:
            raise ValueError("no episode is as long as n_step = %d: there is nothing to fit" % int(n_step))
        return self.train(states, targets, **train_args)

    # -- persistence ----------------------------------------------------------------------------------------------------
    def save(self, path):
        extra = {}
        if self._stats is not None:
            extra = {"mean_in": self._stats[0], "std_in": self._stats[1], "mean_v": self._stats[2], "std_v": self._stats[3]}
        np.savez(path, dim_S=self.dim_S, n_layers=len(self.weights), layers=np.array(self.layer_sizes[1:]),
                 activations=np.array(self.activation_codes),
                 **{"W%d" % i: w for i, w in enumerate(self.weights)}, **{"b%d" % i: b for i, b in enumerate(self.biases)}, **extra)

    @classmethod
    def load(cls, path):
        z = np.load(path)
        m = cls(int(z["dim_S"]), list(z["layers"]), [_ACT_NAME[int(c)] for c in z["activations"]])
        n = int(z["n_layers"])
        m.set_weights([z["W%d" % i] for i in range(n)], [z["b%d" % i] for i in range(n)])
        if "mean_in" in z.files:
            m.set_normalization_stats((z["mean_in"], z["std_in"], z["mean_v"], z["std_v"]))
        return m
