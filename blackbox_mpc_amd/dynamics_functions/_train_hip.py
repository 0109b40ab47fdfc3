"""Training of the Dense stack in hand-written HIP (include/bbmpc.h: bbmpc_trainer_*; csrc/kernels_train.hpp; DESIGN.md
section 8p): `HipDenseTrainer` has `_train_torch.DenseTrainer`'s surface and states the same rule -- drop-remainder
mini-batches through one permutation per epoch, MSE, backprop, Keras TF-2.0 adam / sgd / rmsprop -- as two kernel launches
per step: forward + backward of the batch in one, the update of every parameter in every layout the first one reads in the
other.  The dataset, the permutations of all epochs, the optimizer state and the loss accumulators live on the device; the
losses are read once per fit.  `HipEnsembleTrainer` fits the equally shaped members of an ensemble side by side in the same
two launches per step (the member index is a grid dimension), bit for bit what one `HipDenseTrainer` per member gives.

A log-variance head (Gaussian NLL: ProbabilisticMLP, EnsembleMLP(probabilistic=True)) is fitted by `HipGaussianTrainer` /
`HipGaussianEnsembleTrainer` (bbmpc_trainer_create_gaussian) -- DenseTrainer(..., logvar_head=...)'s
rule in the same kernels' NLL instantiations, W_v and b_v closing the parameter vector.  They are reached with the backend
"hip_nll"; "hip" itself keeps refusing such models, and on a model without a head "hip_nll" is "hip": the same trainers,
launches and bits.  `dense_trainer(backend, ...)` is how every `train(..., backend=...)` of the package picks its trainer."""
import ctypes
import os

import numpy as np

from .. import _lib as L
from . import _train_reg as R

BACKENDS = ("torch", "hip", "hip_nll")
_RULES = {"adam": L.TRAIN_ADAM, "sgd": L.TRAIN_SGD, "rmsprop": L.TRAIN_RMSPROP}
_DECAY_MODES = {"l2": L.TRAIN_DECAY_L2, "decoupled": L.TRAIN_DECAY_DECOUPLED}


def check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError("unknown training backend %r: 'torch' (default), 'hip' or 'hip_nll'" % (backend,))
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


def lds_bytes_gaussian(dims, act_codes):
    """The carve of the kernels' NLL instantiations in bytes (bbmpc_trainer_lds_bytes_gaussian; no device needed)."""
    dims = np.ascontiguousarray(dims, np.int32)
    acts = np.ascontiguousarray(act_codes, np.int32)
    out = ctypes.c_int64(0)
    L.check(L.lib.bbmpc_trainer_lds_bytes_gaussian(len(acts), dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                   acts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(out)))
    return int(out.value)


def lds_bytes_formula_gaussian(dims, act_codes):
    """The same number from the formula DESIGN.md section 8s states: `lds_bytes_formula`'s with T_L more tiles, the head's z:
    4 * (256 * (sum_l T_l + sum over swish layers of T_{l+1} + max_l T_l + T_L) + 1088)."""
    return lds_bytes_formula(dims, act_codes) + 4 * 256 * ((int(dims[-1]) + 15) // 16)


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


class _Regularized:
    """What HipDenseTrainer and HipEnsembleTrainer share of DESIGN.md section 8r: the settings (bbmpc_trainer_set_weight_decay,
    bbmpc_trainer_set_early_stopping; checked here before the library is called, kept by the trainer from fit to fit) and the
    last fit's report (bbmpc_trainer_get_fit_report)."""
    patience, restore_best = 0, False
    _n_val = None                                 # rows of the validation set on the device; None before set_data

    def _require_validation(self, batch_size):
        """Monitoring without a full validation batch is refused here as the library refuses it (a fit before set_data is the
        library's to refuse)."""
        if self._n_val is not None:
            R.require_validation(self.patience, self.restore_best, self._n_val, batch_size)

    def set_weight_decay(self, weight_decay=0.0, decay_mode="l2"):
        """`weight_decay`: a scalar or one value per layer, on the kernels only; 0: off."""
        decay = R.check_options(weight_decay, decay_mode, n_layers=len(self.acts))[0]
        L.check(L.lib.bbmpc_trainer_set_weight_decay(self._t, L.ptr(decay), _DECAY_MODES[decay_mode]))

    def set_early_stopping(self, patience=0, min_delta=0.0, restore_best=False):
        _, _, patience, min_delta, restore_best = R.check_options(patience=patience, min_delta=min_delta, restore_best=restore_best)
        L.check(L.lib.bbmpc_trainer_set_early_stopping(self._t, patience, min_delta, int(restore_best)))
        self.patience, self.restore_best = patience, restore_best

    def _configure(self, weight_decay, decay_mode, patience, min_delta, restore_best):
        """The constructor's options: the library is told only what differs from its defaults."""
        given = R.non_default(weight_decay, decay_mode, patience, min_delta, restore_best)
        if "weight_decay" in given or "decay_mode" in given:
            self.set_weight_decay(weight_decay, decay_mode)
        if given.keys() & {"patience", "min_delta", "restore_best"}:
            self.set_early_stopping(patience, min_delta, restore_best)

    def _fit_report(self, members, epochs):
        if not R.monitoring(self.patience, self.restore_best):      # nothing was tracked: no call into the library
            return np.full((members,), epochs, np.int64), np.full((members,), -1, np.int64), np.full((members,), np.nan)
        epochs_run, best_epoch = np.zeros((members,), np.int32), np.zeros((members,), np.int32)
        best_val = np.zeros((members,), np.float32)
        L.check(L.lib.bbmpc_trainer_get_fit_report(self._t, L.ptr(epochs_run), L.ptr(best_epoch), L.ptr(best_val)))
        return epochs_run.astype(np.int64), best_epoch.astype(np.int64), best_val.astype(np.float64)


class HipDenseTrainer(_Regularized):
    has_logvar_head = False

    def __init__(self, weights, biases, act_codes, device=None, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 rule="adam", rho=0.9, logvar_head=None, weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0,
                 restore_best=False):
        """DenseTrainer's arguments.  The Keras TF-2.0 defaults (beta_1 0.9, beta_2 0.999, epsilon 1e-7, rho 0.9) are the
        only constants the kernels are built with.  weight_decay .. restore_best: `_train_reg`'s options, decided on the
        device (no host synchronisation inside a fit); after a fit `epochs_run`, `best_epoch` (-1: none, or no monitoring)
        and `best_val` describe it."""
        if rule not in _RULES:
            raise ValueError("unknown optimizer rule %r" % (rule,))
        R.check_options(weight_decay, decay_mode, patience, min_delta, restore_best, n_layers=len(weights))
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
        self._configure(weight_decay, decay_mode, patience, min_delta, restore_best)
        self.epochs_run, self.best_epoch, self.best_val = 0, -1, float("nan")

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
        self._n_train, self._n_val = tin.shape[0], vin.shape[0]
        L.check(L.lib.bbmpc_trainer_set_data(self._t, L.ptr(tin), L.ptr(tout), tin.shape[0], L.ptr(vin), L.ptr(vout), vin.shape[0]))

    def fit(self, train_in, train_out, val_in, val_out, epochs, batch_size, permutations=None, generator_seed=None):
        """Returns (train_loss[epochs], val_loss[epochs]); fetch the weights with `numpy_params`."""
        self.set_data(train_in, train_out, val_in, val_out)
        return self.fit_resident(epochs, batch_size, permutations, generator_seed)

    def fit_resident(self, epochs, batch_size, permutations=None, generator_seed=None):
        """`fit` on the rows `set_data` left on the device."""
        epochs = int(epochs)
        self._require_validation(batch_size)
        perms = None
        if permutations is not None:
            perms = np.ascontiguousarray(np.asarray(permutations)[:epochs], np.int32).reshape(epochs, self._n_train)
        seed = int(generator_seed) if generator_seed is not None else int.from_bytes(os.urandom(8), "little")
        tl, vl = np.zeros((epochs,), np.float32), np.zeros((epochs,), np.float32)
        L.check(L.lib.bbmpc_trainer_fit(self._t, epochs, int(batch_size), L.ptr(perms), ctypes.c_uint64(seed & ((1 << 64) - 1)),
                                        L.ptr(tl), L.ptr(vl)))
        report = self._fit_report(1, epochs)
        self.epochs_run, self.best_epoch, self.best_val = int(report[0][0]), int(report[1][0]), float(report[2][0])
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


def member_seed(seed, member):
    """The seed member `member` of an ensemble draws its permutations from when bbmpc_trainer_fit_ensemble is given none:
    seed ^ (0x9E3779B97F4A7C15 * member mod 2^64), so member 0 draws what bbmpc_trainer_fit draws from `seed`."""
    mask = (1 << 64) - 1
    return (int(seed) & mask) ^ ((0x9E3779B97F4A7C15 * int(member)) & mask)


def check_index_bound(n_members, epochs, n_train):
    """bbmpc_trainer_fit_ensemble's bound on the composed index array [n_members][epochs][n_train] (int32 offsets on the
    device), restated: the same error the library raises, before anything is handed to it."""
    count = int(n_members) * int(epochs) * int(n_train)
    if count >= 1 << 31:
        raise L.BBMPCError(L.E_UNSUPPORTED, "trainer: dataset too large: n_members * epochs * n_train = %d index entries, "
                                            "the limit is below %d" % (count, 1 << 31))


class HipEnsembleTrainer(_Regularized):
    """E equally shaped Dense stacks fitted side by side (bbmpc_trainer_create_ensemble; DESIGN.md section 8p, "Members"): the
    member index is a second grid dimension of the training kernels, the dataset is on the device once and a member's
    bootstrap resample is an index map.  Member e's results are, bit for bit, those of a `HipDenseTrainer` fitted on
    `train_in[member_rows[e]]` with member e's start weights and permutations."""
    has_logvar_head = False

    def __init__(self, weights_per_member, biases_per_member, act_codes, device=None, learning_rate=1e-3, rule="adam",
                 weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0, restore_best=False):
        """weight_decay .. restore_best: `_train_reg`'s options, the same for every member; the members monitor, stop and
        restore independently, and after a fit `epochs_run`, `best_epoch`, `best_val` are arrays [E]."""
        if rule not in _RULES:
            raise ValueError("unknown optimizer rule %r" % (rule,))
        R.check_options(weight_decay, decay_mode, patience, min_delta, restore_best, n_layers=len(act_codes))
        self._t = ctypes.c_void_p(None)
        if len(weights_per_member) != len(biases_per_member):
            raise ValueError("one list of biases per list of kernels")
        self._w = [[np.ascontiguousarray(w, np.float32) for w in ws] for ws in weights_per_member]
        self._b = [[np.ascontiguousarray(b, np.float32).reshape(-1) for b in bs] for bs in biases_per_member]
        self.n_members = len(self._w)
        self.acts = [int(a) for a in act_codes]
        first = self._w[0] if self._w else []
        self.dims = ([int(first[0].shape[0])] + [int(w.shape[1]) for w in first]) if first else []
        for e, (ws, bs) in enumerate(zip(self._w, self._b)):
            if len(ws) != len(self.acts) or len(bs) != len(ws):
                raise ValueError("member %d: one activation code and one bias per kernel" % e)
            for l, (w, b) in enumerate(zip(ws, bs)):
                if w.shape != (self.dims[l], self.dims[l + 1]) or b.shape[0] != w.shape[1]:
                    raise ValueError("member %d, layer %d: kernel %s / bias %s do not fit the members' shape %s"
                                     % (e, l, w.shape, b.shape, self.dims))
        self.rule = rule
        dims = np.asarray(self.dims, np.int32)
        acts = np.asarray(self.acts, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.check(L.lib.bbmpc_trainer_create_ensemble(
            ctypes.byref(self._t), _device_index(device), self.n_members, len(self.acts), dims.ctypes.data_as(i32p),
            acts.ctypes.data_as(i32p), _ptr_array([w for ws in self._w for w in ws]), _ptr_array([b for bs in self._b for b in bs]),
            _RULES[rule], float(learning_rate)))
        self._configure(weight_decay, decay_mode, patience, min_delta, restore_best)
        self.epochs_run = np.zeros((self.n_members,), np.int64)
        self.best_epoch = np.full((self.n_members,), -1, np.int64)
        self.best_val = np.full((self.n_members,), np.nan)

    member_seed = staticmethod(member_seed)

    def close(self):
        t, self._t = getattr(self, "_t", None), None
        if t:
            L.lib.bbmpc_trainer_destroy(t)

    __del__ = close

    def set_data(self, train_in, train_out, val_in, val_out, member_rows=None):
        """The shared rows, and per member the training rows it is fitted on (`member_rows` [E][n_train], None: all of them
        in order)."""
        tin, tout = L.f32c(train_in), L.f32c(train_out)
        vin, vout = L.f32c(val_in), L.f32c(val_out)
        tin, tout = tin.reshape(tin.shape[0], -1), tout.reshape(tout.shape[0], -1)
        vin, vout = vin.reshape(vin.shape[0], self.dims[0]), vout.reshape(vout.shape[0], self.dims[-1])
        if tin.shape[1] != self.dims[0] or tout.shape[1] != self.dims[-1] or tin.shape[0] != tout.shape[0] \
                or vin.shape[0] != vout.shape[0]:
            raise ValueError("rows %s -> %s do not fit the network %s" % (tin.shape, tout.shape, self.dims))
        rows = None
        if member_rows is not None:
            rows = np.ascontiguousarray(member_rows, np.int32)
            if rows.shape != (self.n_members, tin.shape[0]):
                raise ValueError("member_rows: [%d][%d] training rows, got %s" % (self.n_members, tin.shape[0], rows.shape))
        self._n_train, self._n_val = tin.shape[0], vin.shape[0]
        L.check(L.lib.bbmpc_trainer_set_data(self._t, L.ptr(tin), L.ptr(tout), tin.shape[0], L.ptr(vin), L.ptr(vout), vin.shape[0]))
        if rows is not None:
            L.check(L.lib.bbmpc_trainer_set_member_rows(self._t, L.ptr(rows)))

    def fit(self, train_in, train_out, val_in, val_out, epochs, batch_size, member_rows=None, permutations=None, generator_seed=None):
        """Returns (train_loss [E, epochs], val_loss [E, epochs]); fetch a member's weights with `numpy_params(member)`.
        `permutations`: [E][epochs][n] (member e's index ITS rows: position pos of an epoch is training row
        member_rows[e][permutations[e][epoch][pos]]) or [epochs][n], shared by the members; None: drawn by the library, member
        e from `member_seed(generator_seed, e)`."""
        self.set_data(train_in, train_out, val_in, val_out, member_rows)
        return self.fit_resident(epochs, batch_size, permutations, generator_seed)

    def fit_resident(self, epochs, batch_size, permutations=None, generator_seed=None):
        """`fit` on the rows (and member rows) `set_data` left on the device."""
        epochs, E, n = int(epochs), self.n_members, self._n_train
        check_index_bound(E, epochs, n)
        self._require_validation(batch_size)
        perms = None
        if permutations is not None:
            p = np.asarray(permutations)
            if p.ndim == 2:                                            # shared by the members
                p = np.broadcast_to(p[None, :epochs], (E, epochs, n))
            elif p.ndim != 3 or p.shape[0] != E:
                raise ValueError("permutations: [%d][epochs][%d] or [epochs][%d], got %s" % (E, n, n, p.shape))
            perms = np.ascontiguousarray(p[:, :epochs], np.int32).reshape(E, epochs, n)
        seed = int(generator_seed) if generator_seed is not None else int.from_bytes(os.urandom(8), "little")
        tl, vl = np.zeros((E, epochs), np.float32), np.zeros((E, epochs), np.float32)
        L.check(L.lib.bbmpc_trainer_fit_ensemble(self._t, epochs, int(batch_size), L.ptr(perms), ctypes.c_uint64(seed & ((1 << 64) - 1)),
                                                 L.ptr(tl), L.ptr(vl)))
        self.epochs_run, self.best_epoch, self.best_val = self._fit_report(E, epochs)
        return tl.astype(np.float64), vl.astype(np.float64)

    def residual_rms(self, val_in, val_out):
        """Per member the per-output RMS of (target - prediction) on the given rows, [E, O]; None without rows."""
        if len(val_in) == 0:
            return None
        vin, vout = L.f32c(val_in), L.f32c(val_out)
        vin, vout = vin.reshape(vin.shape[0], self.dims[0]), vout.reshape(vout.shape[0], self.dims[-1])
        out = np.zeros((self.n_members, self.dims[-1]), np.float32)
        L.check(L.lib.bbmpc_trainer_residual_rms_ensemble(self._t, L.ptr(vin), L.ptr(vout), vin.shape[0], L.ptr(out)))
        return out

    def numpy_params(self, member):
        ws = [np.zeros_like(w) for w in self._w[0]]
        bs = [np.zeros_like(b) for b in self._b[0]]
        L.check(L.lib.bbmpc_trainer_get_member_params(self._t, int(member), _ptr_array(ws), _ptr_array(bs)))
        return ws, bs


def _head_arrays(logvar_head, hidden, out):
    """DenseTrainer's `logvar_head` = (W_v, b_v, min_logvar, max_logvar) as float32 arrays: W_v [hidden][out], b_v [out], the
    bounds [out] (scalars broadcast; the library checks their values)."""
    wv, bv, lo, hi = logvar_head
    wv = np.ascontiguousarray(wv, np.float32)
    bv = np.ascontiguousarray(bv, np.float32).reshape(-1)
    if wv.shape != (hidden, out) or bv.shape != (out,):
        raise ValueError("logvar_head: kernel %s / bias %s do not sit on the last hidden layer (%d) with %d outputs"
                         % (wv.shape, bv.shape, hidden, out))
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (out,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, np.float32), (out,)))
    return wv, bv, lo, hi


def _check_gaussian_options(rule, betas):
    if rule not in _RULES:
        raise ValueError("unknown optimizer rule %r" % (rule,))
    if tuple(float(v) for v in betas) != (0.9, 0.999, 1e-7, 0.9):
        raise ValueError("the hip training backend is built with the Keras TF-2.0 defaults "
                         "(beta_1 0.9, beta_2 0.999, epsilon 1e-7, rho 0.9); use backend='torch' for others")


class HipGaussianTrainer(HipDenseTrainer):
    """HipDenseTrainer's surface for a Dense stack with a log-variance head (bbmpc_trainer_create_gaussian with one member;
    DESIGN.md section 8s): DenseTrainer(..., logvar_head=...)'s rule.  Every loss is the Gaussian NLL, `residual_rms` stays the
    mean network's residual."""
    has_logvar_head = True

    def __init__(self, weights, biases, act_codes, device=None, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 rule="adam", rho=0.9, logvar_head=None, weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0,
                 restore_best=False):
        """logvar_head: (W_v [hidden, out], b_v [out], min_logvar, max_logvar), the bounds scalars or [out]; the other
        arguments are HipDenseTrainer's.  weight_decay decays W_v with the last layer's value and never b_v."""
        _check_gaussian_options(rule, (beta_1, beta_2, epsilon, rho))
        R.check_options(weight_decay, decay_mode, patience, min_delta, restore_best, n_layers=len(weights))
        if logvar_head is None:
            raise ValueError("HipGaussianTrainer needs a logvar_head; HipDenseTrainer fits a network without one")
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
        self._wv, self._bv, self._lo, self._hi = _head_arrays(logvar_head, self.dims[-2], self.dims[-1])
        self.rule = rule
        dims = np.asarray(self.dims, np.int32)
        acts = np.asarray(self.acts, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.check(L.lib.bbmpc_trainer_create_gaussian(
            ctypes.byref(self._t), _device_index(device), 1, len(self._w), dims.ctypes.data_as(i32p), acts.ctypes.data_as(i32p),
            _ptr_array(self._w), _ptr_array(self._b), _ptr_array([self._wv]), _ptr_array([self._bv]), L.ptr(self._lo), L.ptr(self._hi),
            _RULES[rule], float(learning_rate)))
        self._configure(weight_decay, decay_mode, patience, min_delta, restore_best)
        self.epochs_run, self.best_epoch, self.best_val = 0, -1, float("nan")

    @property
    def n_params(self):
        return sum(w.size for w in self._w) + sum(b.size for b in self._b) + self._wv.size + self._bv.size

    def gradients(self, idx):
        """(NLL, [dW_l], [db_l], dW_v, db_v) of the batch made of training rows `idx`, by the step's kernels, nothing
        updated."""
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        g = np.zeros((self.n_params,), np.float32)
        loss = ctypes.c_float(0.0)
        L.check(L.lib.bbmpc_trainer_gradients(self._t, L.ptr(idx), idx.shape[0], L.ptr(g), ctypes.byref(loss)))
        out, o = [], 0
        for a in self._w + self._b + [self._wv, self._bv]:
            out.append(g[o:o + a.size].reshape(a.shape))
            o += a.size
        n = len(self._w)
        return float(loss.value), out[:n], out[n:2 * n], out[2 * n], out[2 * n + 1]

    def numpy_logvar_head(self):
        wv, bv = np.zeros_like(self._wv), np.zeros_like(self._bv)
        L.check(L.lib.bbmpc_trainer_get_logvar_head(self._t, 0, L.ptr(wv), L.ptr(bv)))
        return wv, bv


class HipGaussianEnsembleTrainer(HipEnsembleTrainer):
    """HipEnsembleTrainer's surface for E equally shaped Dense stacks with a log-variance head each
    (bbmpc_trainer_create_gaussian): all members in one launch sequence, member e bit for bit the `HipGaussianTrainer` with its
    start parameters, rows and permutations.  The bounds are shared by the members."""
    has_logvar_head = True

    def __init__(self, weights_per_member, biases_per_member, act_codes, device=None, learning_rate=1e-3, rule="adam",
                 logvar_heads=None, min_logvar=-10.0, max_logvar=0.5, weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0,
                 restore_best=False, beta_1=0.9, beta_2=0.999, epsilon=1e-7, rho=0.9):
        """logvar_heads: per member (W_v [hidden, out], b_v [out]); min_logvar / max_logvar: scalars or [out]."""
        _check_gaussian_options(rule, (beta_1, beta_2, epsilon, rho))
        R.check_options(weight_decay, decay_mode, patience, min_delta, restore_best, n_layers=len(act_codes))
        self._t = ctypes.c_void_p(None)
        if len(weights_per_member) != len(biases_per_member) or logvar_heads is None or len(logvar_heads) != len(weights_per_member):
            raise ValueError("one list of biases and one entry of logvar_heads per list of kernels")
        self._w = [[np.ascontiguousarray(w, np.float32) for w in ws] for ws in weights_per_member]
        self._b = [[np.ascontiguousarray(b, np.float32).reshape(-1) for b in bs] for bs in biases_per_member]
        self.n_members = len(self._w)
        self.acts = [int(a) for a in act_codes]
        first = self._w[0] if self._w else []
        self.dims = ([int(first[0].shape[0])] + [int(w.shape[1]) for w in first]) if first else []
        for e, (ws, bs) in enumerate(zip(self._w, self._b)):
            if len(ws) != len(self.acts) or len(bs) != len(ws):
                raise ValueError("member %d: one activation code and one bias per kernel" % e)
            for l, (w, b) in enumerate(zip(ws, bs)):
                if w.shape != (self.dims[l], self.dims[l + 1]) or b.shape[0] != w.shape[1]:
                    raise ValueError("member %d, layer %d: kernel %s / bias %s do not fit the members' shape %s"
                                     % (e, l, w.shape, b.shape, self.dims))
        heads = [_head_arrays((wv, bv, min_logvar, max_logvar), self.dims[-2], self.dims[-1]) for wv, bv in logvar_heads] \
            if self.dims else []
        self._wv, self._bv = [h[0] for h in heads], [h[1] for h in heads]
        lo = heads[0][2] if heads else np.zeros((0,), np.float32)
        hi = heads[0][3] if heads else np.zeros((0,), np.float32)
        self.rule = rule
        dims = np.asarray(self.dims, np.int32)
        acts = np.asarray(self.acts, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.check(L.lib.bbmpc_trainer_create_gaussian(
            ctypes.byref(self._t), _device_index(device), self.n_members, len(self.acts), dims.ctypes.data_as(i32p),
            acts.ctypes.data_as(i32p), _ptr_array([w for ws in self._w for w in ws]), _ptr_array([b for bs in self._b for b in bs]),
            _ptr_array(self._wv), _ptr_array(self._bv), L.ptr(lo), L.ptr(hi), _RULES[rule], float(learning_rate)))
        self._configure(weight_decay, decay_mode, patience, min_delta, restore_best)
        self.epochs_run = np.zeros((self.n_members,), np.int64)
        self.best_epoch = np.full((self.n_members,), -1, np.int64)
        self.best_val = np.full((self.n_members,), np.nan)

    def numpy_logvar_head(self, member):
        wv, bv = np.zeros_like(self._wv[0]), np.zeros_like(self._bv[0])
        L.check(L.lib.bbmpc_trainer_get_logvar_head(self._t, int(member), L.ptr(wv), L.ptr(bv)))
        return wv, bv


def dense_trainer(backend, weights, biases, act_codes, device, **kwargs):
    """The trainer behind every `train(..., backend=...)`: DenseTrainer for "torch", HipDenseTrainer for "hip" and for
    "hip_nll" on a model without a log-variance head, HipGaussianTrainer for "hip_nll" on one with a head."""
    backend = check_backend(backend)
    if backend == "hip_nll" and kwargs.get("logvar_head") is not None:
        return HipGaussianTrainer(weights, biases, act_codes, device, **kwargs)
    if backend in ("hip", "hip_nll"):
        return HipDenseTrainer(weights, biases, act_codes, device, **kwargs)
    from ._train_torch import DenseTrainer
    return DenseTrainer(weights, biases, act_codes, device, **kwargs)
