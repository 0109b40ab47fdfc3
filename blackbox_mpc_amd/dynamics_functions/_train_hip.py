"""Training of the Dense stack in hand-written HIP (include/bbmpc.h: bbmpc_trainer_*; csrc/kernels_train.hpp; DESIGN.md
section 8p): `HipDenseTrainer` has `_train_torch.DenseTrainer`'s surface and states the same rule -- drop-remainder
mini-batches through one permutation per epoch, MSE, backprop, Keras TF-2.0 adam / sgd / rmsprop -- as two kernel launches
per step: forward + backward of the batch in one, the update of every parameter in every layout the first one reads in the
other.  The dataset, the permutations of all epochs, the optimizer state and the loss accumulators live on the device; the
losses are read once per fit.

Out of scope: a log-variance head (Gaussian NLL) -- ProbabilisticMLP and EnsembleMLP(probabilistic=True) train with the
torch backend.  `dense_trainer(backend, ...)` is how every `train(..., backend=...)` of the package picks its trainer."""
import ctypes
import os

import numpy as np

from .. import _lib as L

BACKENDS = ("torch", "hip")
_RULES = {"adam": L.TRAIN_ADAM, "sgd": L.TRAIN_SGD, "rmsprop": L.TRAIN_RMSPROP}


def check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError("unknown training backend %r: 'torch' (default) or 'hip'" % (backend,))
    return backend


def lds_bytes(dims, act_codes):
    """The step kernel's LDS carve in bytes (bbmpc_trainer_lds_bytes; host arithmetic, no device needed)."""
    dims = np.ascontiguousarray(dims, np.int32)
    acts = np.ascontiguousarray(act_codes, np.int32)
    out = ctypes.c_int64(0)
    L.check(L.lib.bbmpc_trainer_lds_bytes(len(acts), dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          acts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(out)))
    return int(out.value)


def lds_bytes_formula(dims, act_codes):
    """The same number from the formula DESIGN.md section 8p states:
    4 * (256 * (sum_l T_l + sum over swish layers of T_{l+1} + max_l T_l) + 1088), T_l = ceil(dims[l] / 16)."""
    t = [(int(d) + 15) // 16 for d in dims]
    pre = sum(t[l + 1] for l, a in enumerate(act_codes) if a == L.ACT_SWISH)
    return 4 * (256 * (sum(t) + pre + max(t)) + 1088)


def draw_permutation(seed, epoch, n):
    """The permutation bbmpc_trainer_fit draws for `epoch` when it is given none (the generator include/bbmpc.h documents:
    splitmix64 + Fisher-Yates from the top), restated with Python integers."""
    mask = (1 << 64) - 1
    s = (int(seed) ^ (0xD1B54A32D192ED03 * (epoch + 1))) & mask
    out = list(range(n))
    for i in range(n - 1, 0, -1):
        s = (s + 0x9E3779B97F4A7C15) & mask
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        j = (z * (i + 1)) >> 64
        out[i], out[j] = out[j], out[i]
    return np.asarray(out, np.int64)


def _device_index(device):
    if device is None:
        return -1
    if isinstance(device, int):
        return device
    name = str(device)
    if name in ("cuda", "hip"):
        return -1
    if name.startswith("cuda:") or name.startswith("hip:"):
        return int(name.split(":", 1)[1])
    raise ValueError("the hip training backend runs on a GPU: device %r is not one (use backend='torch' to train on the host)" % (device,))


def _ptr_array(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


class HipDenseTrainer:
    has_logvar_head = False

    def __init__(self, weights, biases, act_codes, device=None, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 rule="adam", rho=0.9, logvar_head=None):
        """DenseTrainer's arguments.  The Keras TF-2.0 defaults (beta_1 0.9, beta_2 0.999, epsilon 1e-7, rho 0.9) are the
        only constants the kernels are built with."""
        if rule not in _RULES:
            raise ValueError("unknown optimizer rule %r" % (rule,))
        if logvar_head is not None:
            raise ValueError("the hip training backend fits plain Dense stacks (MSE); a log-variance head (Gaussian NLL) "
                             "trains with backend='torch'")
        if (float(beta_1), float(beta_2), float(epsilon), float(rho)) != (0.9, 0.999, 1e-7, 0.9):
            raise ValueError("the hip training backend is built with the Keras TF-2.0 defaults "
                             "(beta_1 0.9, beta_2 0.999, epsilon 1e-7, rho 0.9); use backend='torch' for others")
        self._t = ctypes.c_void_p(None)
        self._w = [np.ascontiguousarray(w, np.float32) for w in weights]
        self._b = [np.ascontiguousarray(b, np.float32).reshape(-1) for b in biases]
        self.acts = [int(a) for a in act_codes]
        self.dims = [int(self._w[0].shape[0])] + [int(w.shape[1]) for w in self._w]
        for l, (w, b) in enumerate(zip(self._w, self._b)):
            if w.ndim != 2 or w.shape[0] != self.dims[l] or b.shape[0] != w.shape[1]:
                raise ValueError("layer %d: kernel %s / bias %s do not chain" % (l, w.shape, b.shape))
        if len(self.acts) != len(self._w) or len(self._b) != len(self._w):
            raise ValueError("one activation code and one bias per kernel")
        self.rule = rule
        dims = np.asarray(self.dims, np.int32)
        acts = np.asarray(self.acts, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.check(L.lib.bbmpc_trainer_create(ctypes.byref(self._t), _device_index(device), len(self._w), dims.ctypes.data_as(i32p),
                                           acts.ctypes.data_as(i32p), _ptr_array(self._w), _ptr_array(self._b), _RULES[rule],
                                           float(learning_rate)))

    def close(self):
        t, self._t = getattr(self, "_t", None), None
        if t:
            L.lib.bbmpc_trainer_destroy(t)

    __del__ = close

    @property
    def n_params(self):
        return sum(w.size for w in self._w) + sum(b.size for b in self._b)

    def set_data(self, train_in, train_out, val_in, val_out):
        tin, tout = L.f32c(train_in), L.f32c(train_out)
        vin, vout = L.f32c(val_in), L.f32c(val_out)
        tin, tout = tin.reshape(tin.shape[0], -1), tout.reshape(tout.shape[0], -1)
        vin, vout = vin.reshape(vin.shape[0], self.dims[0]), vout.reshape(vout.shape[0], self.dims[-1])
        if tin.shape[1] != self.dims[0] or tout.shape[1] != self.dims[-1] or tin.shape[0] != tout.shape[0] \
                or vin.shape[0] != vout.shape[0]:
            raise ValueError("rows %s -> %s do not fit the network %s" % (tin.shape, tout.shape, self.dims))
        self._n_train = tin.shape[0]
        L.check(L.lib.bbmpc_trainer_set_data(self._t, L.ptr(tin), L.ptr(tout), tin.shape[0], L.ptr(vin), L.ptr(vout), vin.shape[0]))

    def fit(self, train_in, train_out, val_in, val_out, epochs, batch_size, permutations=None, generator_seed=None):
        """Returns (train_loss[epochs], val_loss[epochs]); fetch the weights with `numpy_params`."""
        self.set_data(train_in, train_out, val_in, val_out)
        return self.fit_resident(epochs, batch_size, permutations, generator_seed)

    def fit_resident(self, epochs, batch_size, permutations=None, generator_seed=None):
        """`fit` on the rows `set_data` left on the device."""
        epochs = int(epochs)
        perms = None
        if permutations is not None:
            perms = np.ascontiguousarray(np.asarray(permutations)[:epochs], np.int32).reshape(epochs, self._n_train)
        seed = int(generator_seed) if generator_seed is not None else int.from_bytes(os.urandom(8), "little")
        tl, vl = np.zeros((epochs,), np.float32), np.zeros((epochs,), np.float32)
        L.check(L.lib.bbmpc_trainer_fit(self._t, epochs, int(batch_size), L.ptr(perms), ctypes.c_uint64(seed & ((1 << 64) - 1)),
                                        L.ptr(tl), L.ptr(vl)))
        return tl.astype(np.float64), vl.astype(np.float64)

    def gradients(self, idx):
        """(loss, [dW_l], [db_l]) of the batch made of training rows `idx`, by the step's kernels, nothing updated."""
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        g = np.zeros((self.n_params,), np.float32)
        loss = ctypes.c_float(0.0)
        L.check(L.lib.bbmpc_trainer_gradients(self._t, L.ptr(idx), idx.shape[0], L.ptr(g), ctypes.byref(loss)))
        gw, gb, o = [], [], 0
        for w in self._w:
            gw.append(g[o:o + w.size].reshape(w.shape))
            o += w.size
        for b in self._b:
            gb.append(g[o:o + b.size])
            o += b.size
        return float(loss.value), gw, gb

    def residual_rms(self, val_in, val_out):
        """Per-output RMS of (target - prediction) on the given rows; None without rows."""
        if len(val_in) == 0:
            return None
        vin, vout = L.f32c(val_in), L.f32c(val_out)
        vin, vout = vin.reshape(vin.shape[0], self.dims[0]), vout.reshape(vout.shape[0], self.dims[-1])
        out = np.zeros((self.dims[-1],), np.float32)
        L.check(L.lib.bbmpc_trainer_residual_rms(self._t, L.ptr(vin), L.ptr(vout), vin.shape[0], L.ptr(out)))
        return out

    def numpy_params(self):
        ws = [np.zeros_like(w) for w in self._w]
        bs = [np.zeros_like(b) for b in self._b]
        L.check(L.lib.bbmpc_trainer_get_params(self._t, _ptr_array(ws), _ptr_array(bs)))
        return ws, bs


def dense_trainer(backend, weights, biases, act_codes, device, **kwargs):
    """The trainer behind every `train(..., backend=...)`: DenseTrainer for "torch", HipDenseTrainer for "hip"."""
    if check_backend(backend) == "hip":
        return HipDenseTrainer(weights, biases, act_codes, device, **kwargs)
    from ._train_torch import DenseTrainer
    return DenseTrainer(weights, biases, act_codes, device, **kwargs)
