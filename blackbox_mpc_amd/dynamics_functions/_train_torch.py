"""On-device training of the Dense stack: the counterpart of the reference's
`SystemDynamicsHandler._training_algorithm` (dynamics_handlers/system_dynamics_handler.py:243-290) with
`DeterministicMLP.get_loss` (dynamics_functions/deterministic_mlp.py:53-92, Keras MeanSquaredError) and
`tf.keras.optimizers.Adam` (TF 2.0: lr_t = lr*sqrt(1-b2^t)/(1-b1^t), w -= lr_t*m/(sqrt(v)+1e-7)).

MI355X shape of it: the whole (normalised) dataset lives in HBM, the epoch permutation is drawn on the device, and
one training step -- batch gather, forward, hand-written backward, Adam -- is ~40 tiny kernels on a 26-200-200-20
network, i.e. launch bound: the step is captured once in a HIP graph and replayed per batch (no autograd tape, no
host synchronisation inside an epoch; the loss is accumulated on the device and read once per epoch).
PyTorch-ROCm is plumbing here (hipBLASLt GEMMs, streams, graphs)."""
import os

import numpy as np

from .. import _lib as L


_SELU_ALPHA, _SELU_SCALE = 1.6732632423543772, 1.0507009873554805


def _act(code, x):
    import torch
    F = torch.nn.functional
    if code == L.ACT_TANH:
        return torch.tanh(x)
    if code == L.ACT_RELU:
        return torch.relu(x)
    if code == L.ACT_SIGMOID:
        return torch.sigmoid(x)
    if code == L.ACT_ELU:
        return F.elu(x)
    if code == L.ACT_SELU:
        return F.selu(x)
    if code == L.ACT_SOFTPLUS:
        return F.softplus(x)
    if code == L.ACT_SOFTSIGN:
        return F.softsign(x)
    if code == L.ACT_EXPONENTIAL:
        return torch.exp(x)
    if code == L.ACT_HARD_SIGMOID:
        return torch.clamp(0.2 * x + 0.5, 0.0, 1.0)           # Keras 2.0's, not torch's hardsigmoid
    if code == L.ACT_SWISH:
        return F.silu(x)
    if code == L.ACT_LEAKY_RELU:
        return F.leaky_relu(x, 0.2)                            # tf.nn.leaky_relu's slope
    if code == L.ACT_RELU6:
        return F.relu6(x)
    return x


# activations whose derivative is not a function of the layer output alone: the forward pass keeps their pre-activation
_NEEDS_PRE = (L.ACT_SWISH,)


def _act_grad(code, y, g, z=None):
    """g * f'(x) rebuilt from the layer output y = f(x) (z = x, only for the codes in _NEEDS_PRE)."""
    import torch
    if code == L.ACT_TANH:
        return g * (1.0 - y * y)
    if code == L.ACT_RELU:
        return g * (y > 0).to(g.dtype)
    if code == L.ACT_SIGMOID:
        return g * (y * (1.0 - y))
    if code == L.ACT_ELU:                                      # x > 0 <=> y > 0; e^x = y + 1
        return g * torch.where(y > 0, torch.ones_like(y), y + 1.0)
    if code == L.ACT_SELU:                                     # lambda alpha e^x = y + lambda alpha
        return g * torch.where(y > 0, torch.full_like(y, _SELU_SCALE), y + _SELU_SCALE * _SELU_ALPHA)
    if code == L.ACT_SOFTPLUS:                                 # sigma(x) = 1 - e^-y
        return g * -torch.expm1(-y)
    if code == L.ACT_SOFTSIGN:                                 # 1 / (1 + |x|)^2 = (1 - |y|)^2
        return g * (1.0 - y.abs()).square()
    if code == L.ACT_EXPONENTIAL:
        return g * y
    if code == L.ACT_HARD_SIGMOID:
        return g * (0.2 * ((y > 0) & (y < 1)).to(g.dtype))
    if code == L.ACT_SWISH:                                    # sigma(x) (1 + x (1 - sigma(x))) = s + y (1 - s)
        s = torch.sigmoid(z)
        return g * (s + y * (1.0 - s))
    if code == L.ACT_LEAKY_RELU:
        return g * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.2))
    if code == L.ACT_RELU6:
        return g * ((y > 0) & (y < 6)).to(g.dtype)
    return g


class DenseTrainer:
    def __init__(self, weights, biases, act_codes, device, learning_rate=1e-3, beta_1=0.9, beta_2=0.999,
                 epsilon=1e-7, rule="adam", rho=0.9, logvar_head=None, weight_decay=0.0, decay_mode="l2", patience=0,
                 min_delta=0.0, restore_best=False):
        """rule: "adam" | "sgd" | "rmsprop" -- tf.keras.optimizers.{Adam, SGD, RMSprop}(learning_rate=lr) with their
        TF-2.0 defaults, which is how the reference instantiates `nn_optimizer` (system_dynamics_handler.py:261):
          sgd      w -= lr * g                                              (momentum 0)
          rmsprop  v = rho*v + (1-rho)*g^2 ;  w -= lr * g / (sqrt(v) + eps)   (rho 0.9, momentum 0, eps 1e-7, not centered)
        logvar_head: None, or (W_v [hidden, out], b_v [out], min_logvar, max_logvar) of a ProbabilisticMLP -- a second last
        Dense layer on the last hidden activation.  The loss is then the Gaussian negative log-likelihood
          z = h W_v + b_v;  lv1 = max_lv - softplus(max_lv - z);  lv = min_lv + softplus(lv1 - min_lv)
          loss = mean over the batch's B * out elements of (mu - y)^2 exp(-lv) + lv
        with the backward pass written out like the Dense stack's (dlv/dz = sigmoid(lv1 - min_lv) sigmoid(max_lv - z));
        W_v and b_v join `params`, so every update rule and the captured step cover them.  The bounds are fixed.
        weight_decay / decay_mode / patience / min_delta / restore_best: `_train_reg`'s options.
        Decay is part of the (captured) step; W_v is decayed like any kernel, with the last layer's lambda.  The monitor
        runs on the host after each epoch's validation loss (the NLL with a log-variance head), which this trainer
        reads per epoch anyway.  After a fit: `epochs_run`, `best_epoch` (-1: none, or no monitoring), `best_val`."""
        if rule not in ("adam", "sgd", "rmsprop"):
            raise ValueError("unknown optimizer rule %r" % (rule,))
        from . import _train_reg as R
        self.decay, self.decay_mode, self.patience, self.min_delta, self.restore_best = R.check_options(
            weight_decay, decay_mode, patience, min_delta, restore_best, n_layers=len(weights))
        self.epochs_run, self.best_epoch, self.best_val = 0, -1, float("nan")
        self.rule, self.rho = rule, float(rho)
        import torch
        self.torch = torch
        self.dev = torch.device(device)
        self.acts = list(act_codes)
        self.w = [torch.tensor(np.asarray(w, np.float32), device=self.dev) for w in weights]
        self.b = [torch.tensor(np.asarray(b, np.float32), device=self.dev) for b in biases]
        self.params = self.w + self.b
        self.has_logvar_head = logvar_head is not None
        if self.has_logvar_head:
            wv, bv, lo, hi = logvar_head
            self.wv = torch.tensor(np.asarray(wv, np.float32), device=self.dev)
            self.bv = torch.tensor(np.asarray(bv, np.float32), device=self.dev)
            out = self.bv.shape[0]
            self.min_lv = torch.tensor(np.broadcast_to(np.asarray(lo, np.float32), (out,)).copy(), device=self.dev)
            self.max_lv = torch.tensor(np.broadcast_to(np.asarray(hi, np.float32), (out,)).copy(), device=self.dev)
            if self.wv.shape != (self.w[-1].shape[0], out) or out != self.w[-1].shape[1]:
                raise ValueError("logvar_head: kernel %s does not sit on the last hidden layer %s"
                                 % (tuple(self.wv.shape), tuple(self.w[-1].shape)))
            self.params = self.params + [self.wv, self.bv]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        # (index into params / grads, lambda) of every decayed kernel
        self._decayed = []
        if self.decay is not None:
            self._decayed = [(l, float(lam)) for l, lam in enumerate(self.decay) if lam > 0]
            if self.has_logvar_head and self.decay[-1] > 0:
                self._decayed.append((2 * len(self.w), float(self.decay[-1])))
        self.lr, self.b1, self.b2, self.eps = float(learning_rate), float(beta_1), float(beta_2), float(epsilon)
        # running powers b1^t, b2^t as device scalars so that the step is graph-capturable
        self.b1t = torch.ones((), device=self.dev, dtype=torch.float64)
        self.b2t = torch.ones((), device=self.dev, dtype=torch.float64)
        self.loss_acc = torch.zeros((), device=self.dev, dtype=torch.float32)
        self._graph = None

    # -- one step on (x, y): forward, MSE, backward, Keras-Adam ---------------------------------------------------
    def forward(self, x, pre=None):
        """The layer outputs [x, y1, ..., yL]; `pre`, when given, collects the pre-activations the backward pass needs
        (None for the layers whose derivative follows from y)."""
        ys = [x]
        for w, b, a in zip(self.w, self.b, self.acts):
            z = self.torch.addmm(b, ys[-1], w)
            if pre is not None:
                pre.append(z if a in _NEEDS_PRE else None)
            ys.append(_act(a, z))
        return ys

    @staticmethod
    def _softplus(x):
        """max(x, 0) + log(1 + e^-|x|): csrc/activations.hpp's form, no threshold."""
        return x.clamp(min=0.0) + (-x.abs()).exp().log1p()

    def logvar(self, h):
        """The clamped log-variance of the head on the last hidden activation h, with what the backward pass needs:
        (lv, dlv/dz)."""
        torch = self.torch
        z = torch.addmm(self.bv, h, self.wv)
        lv1 = self.max_lv - self._softplus(self.max_lv - z)
        lv = self.min_lv + self._softplus(lv1 - self.min_lv)
        return lv, torch.sigmoid(lv1 - self.min_lv) * torch.sigmoid(self.max_lv - z)

    def nll(self, x, y):
        """Per-element (mu - y)^2 exp(-lv) + lv of the rows (x, y): [B, out]."""
        ys = self.forward(x)
        lv, _ = self.logvar(ys[-2])
        d = ys[-1] - y
        return d * d * (-lv).exp() + lv

    def _step(self, x, y):
        torch = self.torch
        zs = []
        ys = self.forward(x, zs)
        diff = ys[-1] - y
        n = len(self.w)
        gz = None
        if self.has_logvar_head:
            lv, dlv_dz = self.logvar(ys[n - 1])
            inv = (-lv).exp()
            wsq = diff * diff * inv
            self.loss_acc += (wsq + lv).mean()
            g = diff * inv * (2.0 / diff.numel())
            gz = (1.0 - wsq) * dlv_dz * (1.0 / diff.numel())              # d loss / d z through the soft clamp
        else:
            self.loss_acc += (diff * diff).mean()
            g = diff * (2.0 / diff.numel())
        grads = [None] * (2 * n)
        for l in reversed(range(n)):
            g = _act_grad(self.acts[l], ys[l + 1], g, zs[l])
            grads[l] = ys[l].t() @ g
            grads[n + l] = g.sum(dim=0)
            if l:
                g = g @ self.w[l].t()
                if gz is not None and l == n - 1:                          # the head reads the same hidden activation
                    g = g + gz @ self.wv.t()
        if gz is not None:
            grads = grads + [ys[n - 1].t() @ gz, gz.sum(dim=0)]
        if self._decayed:
            # both modes use the kernels as they are before the step
            if self.decay_mode == "l2":
                for i, lam in self._decayed:
                    grads[i] = torch.add(grads[i], self.params[i], alpha=lam)
                self._rule(grads)
            else:
                before = [self.params[i].clone() for i, _ in self._decayed]
                self._rule(grads)
                for (i, lam), w0 in zip(self._decayed, before):
                    self.params[i].add_(w0, alpha=-(self.lr * lam))
            return
        self._rule(grads)

    def _rule(self, grads):
        torch = self.torch
        if self.rule == "sgd":
            torch._foreach_add_(self.params, grads, alpha=-self.lr)
            return
        if self.rule == "rmsprop":
            torch._foreach_mul_(self.v, self.rho)
            torch._foreach_addcmul_(self.v, grads, grads, value=1.0 - self.rho)
            den = torch._foreach_sqrt(self.v)
            torch._foreach_add_(den, self.eps)
            upd = torch._foreach_div(grads, den)
            torch._foreach_add_(self.params, upd, alpha=-self.lr)
            return
        self.b1t *= self.b1
        self.b2t *= self.b2
        lr_t = (self.lr * torch.sqrt(1.0 - self.b2t) / (1.0 - self.b1t)).to(torch.float32)
        torch._foreach_mul_(self.m, self.b1)
        torch._foreach_add_(self.m, grads, alpha=1.0 - self.b1)
        torch._foreach_mul_(self.v, self.b2)
        torch._foreach_addcmul_(self.v, grads, grads, value=1.0 - self.b2)
        den = torch._foreach_sqrt(self.v)
        torch._foreach_add_(den, self.eps)
        upd = torch._foreach_div(self.m, den)
        torch._foreach_mul_(upd, -lr_t)
        torch._foreach_add_(self.params, upd)

    def _gather_step(self):
        # batch = rows perm[pos : pos + B]; `pos` is a device scalar advanced here so that an epoch is nothing but
        # graph replays
        idx = self._perm.index_select(0, self._ar + self._pos)
        self._pos += self._ar.shape[0]
        self._step(self._din.index_select(0, idx), self._dout.index_select(0, idx))

    def fit(self, train_in, train_out, val_in, val_out, epochs, batch_size, permutations=None, generator_seed=None):
        """Returns (train_loss[epochs], val_loss[epochs]); weights are updated in place (fetch with `numpy_params`)."""
        torch = self.torch
        self._din = torch.as_tensor(np.ascontiguousarray(train_in, np.float32)).to(self.dev)
        self._dout = torch.as_tensor(np.ascontiguousarray(train_out, np.float32)).to(self.dev)
        vin = torch.as_tensor(np.ascontiguousarray(val_in, np.float32)).to(self.dev)
        vout = torch.as_tensor(np.ascontiguousarray(val_out, np.float32)).to(self.dev)
        n = self._din.shape[0]
        nb = n // batch_size                                    # drop_remainder=True (:201-202)
        from . import _train_reg as R
        R.require_validation(self.patience, self.restore_best, vin.shape[0], batch_size)
        monitor = R.Monitor(self.patience, self.min_delta) if R.monitoring(self.patience, self.restore_best) else None
        snapshot = None
        self._perm = torch.zeros((max(n, batch_size),), dtype=torch.int64, device=self.dev)
        self._ar = torch.arange(batch_size, dtype=torch.int64, device=self.dev)
        self._pos = torch.zeros((), dtype=torch.int64, device=self.dev)
        gen = None
        if permutations is None:
            gen = torch.Generator(device=self.dev)
            gen.manual_seed(int(generator_seed) if generator_seed is not None else int.from_bytes(os.urandom(4), "little"))
        use_graph = self.dev.type == "cuda" and nb > 0 and os.environ.get("BBMPC_TRAIN_GRAPH", "1") != "0"
        self._graph = None                      # the graph bakes in this call's dataset / index buffers: capture per fit
        if use_graph:
            # warm-up on a side stream (allocator + hipBLASLt workspaces), state restored afterwards, then capture
            state = self.params + self.m + self.v + [self.b1t, self.b2t, self.loss_acc, self._pos]
            snap = [t.clone() for t in state]
            s = torch.cuda.Stream(device=self.dev)
            s.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(s):
                for _ in range(3):
                    self._pos.zero_()
                    self._gather_step()
            torch.cuda.current_stream(self.dev).wait_stream(s)
            self._graph = torch.cuda.CUDAGraph()
            self._pos.zero_()
            with torch.cuda.graph(self._graph):
                self._gather_step()
            for t, c in zip(state, snap):
                t.copy_(c)
        tl, vl = np.full((epochs,), np.nan), np.full((epochs,), np.nan)
        self.epochs_run = epochs
        for e in range(epochs):
            if permutations is not None:
                perm = torch.as_tensor(np.asarray(permutations[e], np.int64)).to(self.dev)
            else:
                perm = torch.randperm(n, generator=gen, device=self.dev)
            self.loss_acc.zero_()
            self._perm[:n].copy_(perm)
            self._pos.zero_()
            for bi in range(nb):
                if use_graph:
                    self._graph.replay()
                else:
                    self._gather_step()
            if nb:
                tl[e] = float(self.loss_acc.item()) / nb
            nvb = vin.shape[0] // batch_size
            if nvb:
                if self.has_logvar_head:
                    with torch.no_grad():
                        d = self.nll(vin[:nvb * batch_size], vout[:nvb * batch_size]).reshape(nvb, -1)
                    vl[e] = float(d.mean(dim=1).mean().item())      # mean of per-batch NLLs
                else:
                    pv = self.forward(vin[:nvb * batch_size])[-1]
                    d = (pv - vout[:nvb * batch_size]).reshape(nvb, -1)
                    vl[e] = float((d * d).mean(dim=1).mean().item())    # mean of per-batch MSEs (:276-284)
            if monitor is not None:
                improved, stop = monitor.update(e, vl[e])
                if improved and self.restore_best:
                    snapshot = [p.clone() for p in self.params]
                if stop:
                    self.epochs_run = e + 1
                    break
        self.best_epoch, self.best_val = (monitor.best_epoch, monitor.best_val) if monitor is not None else (-1, float("nan"))
        if snapshot is not None:                                # weights only: m, v and the powers stay
            for p, s in zip(self.params, snapshot):
                p.copy_(s)
        return tl, vl

    def residual_rms(self, val_in, val_out):
        """Per-output RMS of (target - prediction) on the given rows, on the training device; None without rows."""
        torch = self.torch
        if len(val_in) == 0:
            return None
        vin = torch.as_tensor(np.ascontiguousarray(val_in, np.float32)).to(self.dev)
        vout = torch.as_tensor(np.ascontiguousarray(val_out, np.float32)).to(self.dev)
        with torch.no_grad():
            d = vout - self.forward(vin)[-1]
            return torch.sqrt((d * d).mean(dim=0)).cpu().numpy().astype(np.float32)

    def numpy_logvar_head(self):
        return self.wv.detach().cpu().numpy(), self.bv.detach().cpu().numpy()

    def numpy_params(self):
        return [w.detach().cpu().numpy() for w in self.w], [b.detach().cpu().numpy() for b in self.b]
