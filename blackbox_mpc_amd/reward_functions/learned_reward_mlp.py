"""LearnedRewardMLP -- a reward network r(s_t, a_t, s_{t+1}) fitted from the reward samples an environment returns, for
users whose reward is not a known function (MBPO, Dreamer and TD-MPC fit one next to the dynamics).

A weights container like DeterministicMLP: Dense kernels [in, out] + biases, Keras default init, one output.  At planning
time the network runs on the matrix cores over the states the learned-model rollouts produce (BBMPC_REW_MLP,
bbmpc_set_reward_mlp; csrc/kernels_reward_mlp.hpp); `train` fits it with dynamics_functions/_train_torch.py, the trainer of
SystemDynamicsHandler.train.  `__call__(current_state, actions, next_state)` evaluates it on NumPy arrays, so the object is
also a reward function in the reference's sense (trajectory_evaluators/deterministic.py:65-66)."""
import numpy as np

from .. import _lib as L
from ..dynamics_functions.deterministic_mlp import _ACT_NAME, _act_code

_SELU_ALPHA, _SELU_SCALE = 1.6732632423543772, 1.0507009873554805
_INPUT_BITS = {"s": L.REW_MLP_IN_STATE, "a": L.REW_MLP_IN_ACTION, "n": L.REW_MLP_IN_NEXT_STATE}


def input_mask(inputs):
    """"sas" / "sa" / "s'" ... -> bbmpc_set_reward_mlp's input_mask.  The letters are read in order: `s` is s_t, `a` is
    a_t, and an `s` behind either of them -- or spelt s' -- is s_{t+1}; an int is taken as the mask itself."""
    if isinstance(inputs, (int, np.integer)):
        mask = int(inputs)
    else:
        mask, seen = 0, ""
        text = str(inputs).lower().replace("s'", "n")
        for ch in text:
            if ch not in "san":
                raise ValueError("inputs must be made of s, a and s' (e.g. 'sas', 'sa', \"s'\"), got %r" % (inputs,))
            if ch == "s" and seen:                   # an s that is not the first letter: the next state
                ch = "n"
            if _INPUT_BITS[ch] & mask or (seen and "san".index(ch) < "san".index(seen[-1])):
                raise ValueError("inputs must name s, a, s' at most once each and in that order, got %r" % (inputs,))
            mask |= _INPUT_BITS[ch]
            seen += ch
    if not 1 <= mask <= 7:
        raise ValueError("inputs must select at least one of s, a, s', got %r" % (inputs,))
    return mask


def numpy_activation(code, x):
    """BBMPC_ACT_* code on a float64 array: the definitions of csrc/activations.hpp."""
    if code == L.ACT_TANH:
        return np.tanh(x)
    if code == L.ACT_RELU:
        return np.maximum(x, 0.0)
    if code == L.ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-x))
    if code == L.ACT_ELU:
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    if code == L.ACT_SELU:
        return _SELU_SCALE * np.where(x > 0, x, _SELU_ALPHA * np.expm1(np.minimum(x, 0.0)))
    if code == L.ACT_SOFTPLUS:
        return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    if code == L.ACT_SOFTSIGN:
        return x / (1.0 + np.abs(x))
    if code == L.ACT_EXPONENTIAL:
        return np.exp(x)
    if code == L.ACT_HARD_SIGMOID:
        return np.clip(0.2 * x + 0.5, 0.0, 1.0)
    if code == L.ACT_SWISH:
        return x / (1.0 + np.exp(-x))
    if code == L.ACT_LEAKY_RELU:
        return np.maximum(x, 0.2 * x)
    if code == L.ACT_RELU6:
        return np.minimum(np.maximum(x, 0.0), 6.0)
    return x


class LearnedRewardMLP:
    _bbmpc_reward_kind = L.REW_MLP

    def __init__(self, dim_S, dim_U, layers, activations, inputs="sas", seed=None, name=None):
        """layers: the Dense widths behind the input, ending in 1 (e.g. [200, 200, 1]); activations: one per Dense layer
        (names or callables, as DeterministicMLP takes them).  inputs: which of s_t, a_t, s_{t+1} the network sees --
        "sas" (all three), "sa", "s'", ... -- concatenated in that order."""
        self.name = name
        self.dim_S, self.dim_U = int(dim_S), int(dim_U)
        self.input_mask = input_mask(inputs)
        self.dim_in = ((self.dim_S if self.input_mask & 1 else 0) + (self.dim_U if self.input_mask & 2 else 0)
                       + (self.dim_S if self.input_mask & 4 else 0))
        widths = [int(v) for v in layers]
        if not widths or widths[-1] != 1:
            raise ValueError("a reward network ends in one output: layers[-1] must be 1, got %r" % (layers,))
        if len(activations) != len(widths):
            raise ValueError("need one activation per Dense layer")
        self.layer_sizes = [self.dim_in] + widths
        self.activation_codes = [_act_code(a) for a in activations]
        rng = np.random.default_rng(seed)
        self.weights, self.biases = [], []
        for i in range(1, len(self.layer_sizes)):
            fan_in, fan_out = self.layer_sizes[i - 1], self.layer_sizes[i]
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            self.weights.append(rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32))
            self.biases.append(np.zeros((fan_out,), np.float32))
        self._stats = None                  # (mean_in [D], std_in [D], mean_r [1], std_r [1]) once trained / set
        self._version = 0
        self._data = None                   # rows collected by train_on_rollouts

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
        """stats = (mean_in [D], std_in [D], mean_r, std_r) or None (an un-normalised network)."""
        if stats is None:
            self._stats = None
        else:
            mi, si, mr, sr = [np.asarray(s, np.float32).reshape(-1) for s in stats]
            if mi.shape != (self.dim_in,) or si.shape != (self.dim_in,) or mr.shape != (1,) or sr.shape != (1,):
                raise ValueError("stats must be (mean_in [%d], std_in [%d], mean_r [1], std_r [1])" % (self.dim_in, self.dim_in))
            self._stats = (mi.copy(), si.copy(), mr.copy(), sr.copy())
        self._version += 1

    def normalization_stats(self):
        return self._stats

    # -- evaluation on the host -----------------------------------------------------------------------------------------
    def assemble_inputs(self, current_state, actions, next_state):
        """The network's input rows [B, D]: the blocks input_mask selects, in the order s_t, a_t, s_{t+1}."""
        blocks = []
        if self.input_mask & 1:
            blocks.append(np.asarray(current_state).reshape(-1, self.dim_S))
        if self.input_mask & 2:
            blocks.append(np.asarray(actions).reshape(-1, self.dim_U))
        if self.input_mask & 4:
            blocks.append(np.asarray(next_state).reshape(-1, self.dim_S))
        return np.concatenate(blocks, axis=1)

    def __call__(self, current_state, actions, next_state):
        """reward_function(current_state [B,S], actions [B,U], next_state [B,S]) -> [B] float32, computed in float64 on the
        host: normalise as SystemDynamicsHandler.process_input does, the Dense stack, y * std_r + mean_r."""
        x = self.assemble_inputs(current_state, actions, next_state).astype(np.float64)
        if self._stats is not None:
            x = (x - self._stats[0].astype(np.float64)) / (self._stats[1].astype(np.float64) + np.float64(np.float32(1e-7)))
        for w, b, a in zip(self.weights, self.biases, self.activation_codes):
            x = numpy_activation(a, x @ w.astype(np.float64) + b.astype(np.float64))
        y = x[:, 0]
        if self._stats is not None:
            y = y * np.float64(self._stats[3][0]) + np.float64(self._stats[2][0])
        return y.astype(np.float32)

    # -- training -------------------------------------------------------------------------------------------------------
    def train(self, states, actions, next_states, rewards, epochs=30, batch_size=128, learning_rate=1e-3,
              validation_split=0.2, device=None, seed=None, normalize=True, backend="torch", *, weight_decay=0.0, decay_mode="l2",
              patience=0, min_delta=0.0, restore_best=False):
        """Fit MSE on normalised targets with Keras-Adam (dynamics_functions/_train_torch.DenseTrainer, on `device`:
        the GPU when PyTorch sees one, else the CPU).  states / next_states [B,S], actions [B,U], rewards [B].  The
        statistics are refreshed from exactly these rows and the version is bumped, so every engine that holds the network
        uploads it again before its next computation.  Returns (train_loss [epochs], validation_loss [epochs]).
        backend: "torch" (the default), "hip" or "hip_nll" (here the same as "hip") -- the hand-written training kernels
        (dynamics_functions/_train_hip.HipDenseTrainer; GPU only, permutations drawn by the library from `seed`).
        weight_decay / decay_mode / patience / min_delta / restore_best (keyword-only): weight decay on the kernels, early
        stopping on the validation loss and best-weights restore (dynamics_functions/_train_reg.py),
        handed to the trainer only where they differ from the defaults; `epochs_run` / `best_epoch` record the fit."""
        from ..dynamics_functions._train_hip import check_backend, dense_trainer
        from ..dynamics_functions._train_reg import non_default
        check_backend(backend)
        reg = non_default(weight_decay, decay_mode, patience, min_delta, restore_best)
        x = self.assemble_inputs(states, actions, next_states).astype(np.float32)
        y = np.asarray(rewards, np.float32).reshape(-1, 1)
        if x.shape[0] != y.shape[0]:
            raise ValueError("%d input rows but %d rewards" % (x.shape[0], y.shape[0]))
        if normalize:
            stats = (x.mean(axis=0), x.std(axis=0), y.mean(axis=0), y.std(axis=0))
            stats = tuple(np.asarray(s, np.float32) for s in stats)
            xn = (x - stats[0]) / (stats[1] + np.float32(1e-7))
            sr = stats[3] if stats[3][0] > 0 else np.ones((1,), np.float32)          # constant rewards: targets stay centred
            stats = (stats[0], stats[1], stats[2], sr)
            yn = (y - stats[2]) / sr
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

    def train_on_rollouts(self, traj_obs, traj_acs, traj_rews, **train_args):
        """Add the episodes perform_rollouts returned (observations [T+1,A,S], actions [T,A,U], rewards [T,A] each) to the
        rows collected so far and refit on all of them."""
        rows = [[], [], [], []]
        for obs, acs, rews in zip(traj_obs, traj_acs, traj_rews):
            obs = np.asarray(obs, np.float32)
            acs = np.asarray(acs, np.float32).reshape(obs.shape[0] - 1, -1, self.dim_U)
            rows[0].append(obs[:-1].reshape(-1, self.dim_S))
            rows[1].append(acs.reshape(-1, self.dim_U))
            rows[2].append(obs[1:].reshape(-1, self.dim_S))
            rows[3].append(np.asarray(rews, np.float32).reshape(-1))
        new = [np.concatenate(r, axis=0) for r in rows]
        self._data = new if self._data is None else [np.concatenate([o, n], axis=0) for o, n in zip(self._data, new)]
        return self.train(*self._data, **train_args)

    # -- persistence ----------------------------------------------------------------------------------------------------
    def save(self, path):
        extra = {}
        if self._stats is not None:
            extra = {"mean_in": self._stats[0], "std_in": self._stats[1], "mean_r": self._stats[2], "std_r": self._stats[3]}
        np.savez(path, dim_S=self.dim_S, dim_U=self.dim_U, input_mask=self.input_mask, n_layers=len(self.weights),
                 layers=np.array(self.layer_sizes[1:]), activations=np.array(self.activation_codes),
                 **{"W%d" % i: w for i, w in enumerate(self.weights)}, **{"b%d" % i: b for i, b in enumerate(self.biases)}, **extra)

    @classmethod
    def load(cls, path):
        z = np.load(path)
        m = cls(int(z["dim_S"]), int(z["dim_U"]), list(z["layers"]), [_ACT_NAME[int(c)] for c in z["activations"]],
                inputs=int(z["input_mask"]))
        n = int(z["n_layers"])
        m.set_weights([z["W%d" % i] for i in range(n)], [z["b%d" % i] for i in range(n)])
        if "mean_in" in z.files:
            m.set_normalization_stats((z["mean_in"], z["std_in"], z["mean_r"], z["std_r"]))
        return m
