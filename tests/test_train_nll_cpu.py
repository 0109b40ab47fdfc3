"""The Gaussian-NLL path of the HIP trainer without a GPU: the float64 rule the GPU tests compare
against (tests/train_nll_util.py) is checked against float64 autograd and against the float32 DenseTrainer, the conditions
the GPU cases rely on hold, "hip_nll" is a backend that is "hip" on a model without a head, and the C ABI declares, exports
and binds the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import train_hip_util as U
from tests import train_nll_util as N
from tests.test_gpu_activations import CODE
from tests.test_train_cpu import _episodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NLL_SYMBOLS = ["bbmpc_trainer_create_gaussian", "bbmpc_trainer_get_logvar_head", "bbmpc_trainer_lds_bytes_gaussian"]
CASES = [(net, B) for net in sorted(N.NETS) for B in N.GRAD_BATCHES]


# ---- 1. the float64 rule against autograd -------------------------------------------------------------------------------
@pytest.mark.parametrize("net,B", CASES)
def test_nll_and_grads_is_the_autograd_gradient_of_the_formulas(net, B):
    """float64 against float64: rtol 1e-10, per element, on every GPU gradient case (a swish layer below the head's input in
    7-20-33-5, L = 1 in 5-3)."""
    import torch
    from blackbox_mpc_amd.dynamics_functions import _train_torch as TT
    ws, bs, acts, head, x, y, idx = N.gradient_case(net, B)
    codes = [CODE[a] for a in acts]
    loss, gw, gb, gwv, gbv = N.nll_and_grads(ws, bs, acts, head, x[idx], y[idx])
    p64 = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in ws + bs + [head[0], head[1]]]
    n = len(ws)
    h = torch.tensor(x[idx].astype(np.float64))
    for i in range(n):
        if i == n - 1:
            z = h @ p64[2 * n] + p64[2 * n + 1]
        h = TT._act(codes[i], h @ p64[i] + p64[n + i])
    sp = TT.DenseTrainer._softplus
    lo, hi = torch.tensor(head[2].astype(np.float64)), torch.tensor(head[3].astype(np.float64))
    lv = lo + sp(hi - sp(hi - z) - lo)
    ref = ((h - torch.tensor(y[idx].astype(np.float64))) ** 2 * torch.exp(-lv) + lv).mean()
    ref.backward()
    np.testing.assert_allclose(loss, float(ref.detach()), rtol=1e-10)
    for got, p in zip(gw + gb + [gwv, gbv], p64):
        assert np.all(np.isfinite(got)) and np.abs(p.grad.numpy()).max() > 1e-5
        np.testing.assert_allclose(got, p.grad.numpy(), rtol=1e-10, atol=0)


# ---- 2. the float64 loop against the float32 DenseTrainer ---------------------------------------------------------------
@pytest.mark.parametrize("rule,lr", N.FIT_RULES)
def test_train_nll_is_the_dense_trainers_rule(rule, lr):
    """tests/test_train_cpu.py's tolerances: parameters atol 3e-4, losses rtol 2e-4 / atol 1e-6."""
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer
    ws, bs, acts, head, tin, tout, vin, vout, perms = N.fit_case("7-20-33-5", seed=20)
    kw = dict(weight_decay=[0.0, 0.0, 0.5], decay_mode="decoupled") if rule == "adam" else {}
    tr = DenseTrainer(ws, bs, [CODE[a] for a in acts], "cpu", learning_rate=lr, rule=rule, logvar_head=head, **kw)
    tl, vl = tr.fit(tin, tout, vin, vout, N.FIT_EPOCHS, N.FIT_BATCH, permutations=perms)
    w, b, hv, wtl, wvl, _ = N.train_nll(ws, bs, acts, head, tin, tout, vin, vout, perms, N.FIT_BATCH, learning_rate=lr, rule=rule, **kw)
    got = tr.numpy_params()[0] + tr.numpy_params()[1] + list(tr.numpy_logvar_head())
    for g, want in zip(got, w + b + list(hv)):
        np.testing.assert_allclose(g, want, rtol=0, atol=3e-4)
    np.testing.assert_allclose(tl, wtl, rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(vl, wvl, rtol=2e-4, atol=1e-6)
    assert np.all(np.isfinite(wvl)) and not np.allclose(hv[0], head[0], atol=1e-3)


# ---- 3. / 4. the conditions the GPU cases rely on -----------------------------------------------------------------------
@pytest.mark.parametrize("net,B", CASES)
def test_every_gradient_case_meets_all_three_regimes_of_the_clamp(net, B):
    ws, bs, acts, head, x, y, idx = N.gradient_case(net, B)
    above, below = N.clamp_shares(ws, bs, acts, head, x[idx])
    assert 0.02 < above < 0.9 and 0.02 < below < 0.9, (above, below)
    assert np.all(head[2] < head[3]) and len(set(head[2].tolist())) == len(head[2])          # per-dimension bounds
    out = N.nll_and_grads(ws, bs, acts, head, x[idx], y[idx])
    assert np.isfinite(out[0]) and all(np.all(np.isfinite(g)) for g in out[1] + out[2] + [out[3], out[4]])


def test_the_rising_case_rises():
    """What the early-stopping GPU case is built for: the float64 validation NLL is lowest after the first epoch and each
    later one is above it by more than 1 % -- float32 cannot order them otherwise."""
    c = N.rising_case()
    free = N.train_nll(*c[:8], c[8], N.FIT_BATCH, rule=N.RISING["rule"], learning_rate=N.RISING["learning_rate"])
    vl = free[4]
    assert np.all(np.isfinite(vl)) and np.all(vl[1:] > 1.01 * vl[0]), vl
    w, b, hv, tl, svl, rep = N.train_nll(*c[:8], c[8], N.FIT_BATCH, **N.RISING)
    assert rep["epochs_run"] == 2 and rep["best_epoch"] == 0 and rep["best_val"] == vl[0]
    assert np.all(np.isnan(svl[2:])) and np.all(np.isnan(tl[2:])) and np.array_equal(svl[:2], vl[:2])
    first = N.train_nll(*c[:8], c[8][:1], N.FIT_BATCH, rule=N.RISING["rule"], learning_rate=N.RISING["learning_rate"])
    np.testing.assert_array_equal(hv[0], first[2][0])                                        # the first epoch's head, restored


# ---- 5. the backend -----------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for a trainer class: records how it was built and fails the fit recognisably."""
    made = []

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs
        type(self).made.append(self)

    def fit(self, *a, **k):
        raise RuntimeError("recorded")

    def close(self):
        pass


def _handler(fn):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    return SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn)


def _norm(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [_norm(a) for a in v]
    if isinstance(v, dict):
        return {k: _norm(a) for k, a in v.items()}
    return v


def _built(args, kwargs):
    """A constructor call in a comparable form."""
    return _norm(args), _norm(kwargs)


def test_hip_nll_is_a_backend_and_is_hip_on_models_without_a_head(built_lib, monkeypatch):
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    from blackbox_mpc_amd.dynamics_functions.probabilistic_mlp import ProbabilisticMLP
    assert T.BACKENDS == ("torch", "hip", "hip_nll") and T.check_backend("hip_nll") == "hip_nll"
    with pytest.raises(ValueError, match="bogus"):
        T.check_backend("bogus")
    obs, acs, rews = _episodes(1, 20, 2, 0)
    dense, ens, gauss, gens = (type("Dense", (_Recorder,), {"made": []}), type("Ens", (_Recorder,), {"made": []}),
                               type("Gauss", (_Recorder,), {"made": []}), type("GaussEns", (_Recorder,), {"made": []}))
    monkeypatch.setattr(T, "HipDenseTrainer", dense)
    monkeypatch.setattr(T, "HipEnsembleTrainer", ens)
    monkeypatch.setattr(T, "HipGaussianTrainer", gauss)
    monkeypatch.setattr(T, "HipGaussianEnsembleTrainer", gens)
    # models without a head: "hip_nll" builds exactly what "hip" builds
    for make, cls in ((lambda: DeterministicMLP([4, 8, 3], ["tanh", None], seed=0), dense),
                      (lambda: EnsembleMLP([4, 8, 3], ["tanh", None], num_members=2, seed=0), ens)):
        calls = []
        for backend in ("hip", "hip_nll"):
            cls.made = []
            with pytest.raises(RuntimeError, match="recorded"):
                _handler(make()).train(obs, acs, rews, epochs=2, batch_size=8, learning_rate=3e-3, seed=1, backend=backend,
                                       weight_decay=0.25)
            assert len(cls.made) == 1 and not gauss.made and not gens.made
            calls.append(_built(cls.made[0].args, cls.made[0].kwargs))
        assert calls[0] == calls[1]
    t = T.dense_trainer("hip_nll", [np.zeros((4, 3), F)], [np.zeros((3,), F)], [0], None, logvar_head=None, learning_rate=1e-3)
    assert type(t) is dense and t.kwargs["logvar_head"] is None
    # the reward / value / policy models go through dense_trainer too
    from blackbox_mpc_amd.policy_functions.learned_policy_mlp import LearnedPolicyMLP
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP
    from blackbox_mpc_amd.value_functions.learned_value_mlp import LearnedValueMLP
    rng = np.random.default_rng(0)
    s, a, s2, r = rng.normal(size=(40, 3)), rng.normal(size=(40, 1)), rng.normal(size=(40, 3)), rng.normal(size=(40,))
    for run in (lambda b: LearnedRewardMLP(3, 1, [8, 1], ["tanh", None], seed=0).train(s, a, s2, r, epochs=1, seed=0, backend=b),
                lambda b: LearnedValueMLP(3, [8, 1], ["tanh", None], seed=0).train(s, r, epochs=1, seed=0, backend=b),
                lambda b: LearnedValueMLP(3, [8, 1], ["tanh", None], seed=0).train_on_rollouts(obs, rews, 2, epochs=1, seed=0, backend=b),
                lambda b: LearnedPolicyMLP(3, 1, [8, 1], ["tanh", None], seed=0).train(s, a, epochs=1, seed=0, backend=b),
                lambda b: LearnedPolicyMLP(3, 1, [8, 1], ["tanh", None], seed=0).train_on_rollouts(obs, acs, epochs=1, seed=0, backend=b)):
        calls = []
        for backend in ("hip", "hip_nll"):
            dense.made = []
            with pytest.raises(RuntimeError, match="recorded"):
                run(backend)
            calls.append(_built(dense.made[0].args, dense.made[0].kwargs))
        assert calls[0] == calls[1]
    # models with a head: one Gaussian trainer; ONE ensemble trainer for all members, with their heads and shared bounds
    gauss.made, gens.made, dense.made, ens.made = [], [], [], []
    fn = ProbabilisticMLP([4, 8, 3], ["tanh", None], seed=0, min_logvar=-3.0, max_logvar=[0.5, 0.25, 0.0])
    with pytest.raises(RuntimeError, match="recorded"):
        _handler(fn).train(obs, acs, rews, epochs=1, batch_size=8, backend="hip_nll")
    assert len(gauss.made) == 1 and not dense.made
    wv, bv, lo, hi = gauss.made[0].kwargs["logvar_head"]
    np.testing.assert_array_equal(wv, fn.logvar_weights)
    np.testing.assert_array_equal(hi, np.asarray([0.5, 0.25, 0.0], F))
    fn = EnsembleMLP([4, 8, 3], ["tanh", None], num_members=3, seed=0, probabilistic=True)
    with pytest.raises(RuntimeError, match="recorded"):
        _handler(fn).train(obs, acs, rews, epochs=1, batch_size=8, backend="hip_nll")
    assert len(gens.made) == 1 and not ens.made and len(gauss.made) == 1
    heads = gens.made[0].kwargs["logvar_heads"]
    assert len(heads) == 3
    for (wv, bv), m in zip(heads, fn.members):
        np.testing.assert_array_equal(wv, m.logvar_weights)
    np.testing.assert_array_equal(gens.made[0].kwargs["min_logvar"], fn.members[0].min_logvar)


def test_the_hip_backend_still_refuses_models_with_a_head(built_lib):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    from blackbox_mpc_amd.dynamics_functions.probabilistic_mlp import ProbabilisticMLP
    obs, acs, rews = _episodes(1, 10, 2, 0)
    for fn in (ProbabilisticMLP([4, 8, 3], ["tanh", None], seed=0),
               EnsembleMLP([4, 8, 3], ["tanh", None], num_members=2, seed=0, probabilistic=True)):
        with pytest.raises(ValueError, match="backend='torch'"):
            _handler(fn).train(obs, acs, rews, epochs=1, batch_size=8, backend="hip")
    ws, bs = U.params((4, 8, 3), seed=0)
    with pytest.raises(ValueError, match="backend='torch'"):
        HipDenseTrainer(ws, bs, [1, 0], logvar_head=(np.zeros((8, 3), F), np.zeros((3,), F), -10.0, 0.5))


def test_python_refusals_of_the_gaussian_trainers_come_before_the_library(built_lib):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipGaussianEnsembleTrainer, HipGaussianTrainer
    ws, bs = U.params((4, 8, 3), seed=0)
    good = (np.zeros((8, 3), F), np.zeros((3,), F), -10.0, 0.5)
    with pytest.raises(ValueError, match="logvar_head"):
        HipGaussianTrainer(ws, bs, [1, 0], logvar_head=(np.zeros((3, 8), F), np.zeros((3,), F), -10.0, 0.5))
    with pytest.raises(ValueError, match="logvar_head"):
        HipGaussianTrainer(ws, bs, [1, 0], logvar_head=None)
    with pytest.raises(ValueError, match="backend='torch'"):
        HipGaussianTrainer(ws, bs, [1, 0], logvar_head=good, beta_1=0.8)
    with pytest.raises(ValueError, match="backend='torch'"):
        HipGaussianEnsembleTrainer([ws], [bs], [1, 0], logvar_heads=[good[:2]], epsilon=1e-8)
    with pytest.raises(ValueError, match="rule"):
        HipGaussianTrainer(ws, bs, [1, 0], logvar_head=good, rule="adagrad")
    with pytest.raises(ValueError, match="logvar_head"):
        HipGaussianEnsembleTrainer([ws], [bs], [1, 0], logvar_heads=[(np.zeros((8, 4), F), np.zeros((4,), F))])


# ---- 6. the C ABI ---------------------------------------------------------------------------------------------------------
def test_the_gaussian_entry_points_are_declared_and_bound(built_lib):
    from blackbox_mpc_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text) and L.lib.bbmpc_abi_version() == 4      # entry points added
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(built_lib)
    for name in NLL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(L.lib, name).argtypes is not None, name
    assert len(L.lib.bbmpc_trainer_create_gaussian.argtypes) == 14 and len(L.lib.bbmpc_trainer_get_logvar_head.argtypes) == 4
    vp = ctypes.c_void_p
    assert L.lib.bbmpc_trainer_get_logvar_head(None, 0, None, None) == L.E_INVALID and "trainer" in L.lib.bbmpc_last_error().decode()
    out = vp(None)
    i32p = ctypes.POINTER(ctypes.c_int32)
    d, a = np.asarray([4, 8, 3], np.int32), np.asarray([1, 0], np.int32)
    for E, want in ((9, L.E_UNSUPPORTED), (0, L.E_UNSUPPORTED), (2, L.E_INVALID)):           # member count; then the null arrays
        assert L.lib.bbmpc_trainer_create_gaussian(ctypes.byref(out), -1, E, 2, d.ctypes.data_as(i32p), a.ctypes.data_as(i32p), None, None,
                                                   None, None, None, None, 1, 1e-3) == want
        assert "trainer" in L.lib.bbmpc_last_error().decode() and not out.value


@pytest.mark.parametrize("dims,acts", [((26, 200, 200, 20), (1, 1, 0)), ((26, 500, 500, 500, 20), (1, 1, 1, 0)),
                                       ((7, 20, 33, 5), (10, 1, 0)), ((5, 3), (0,))])
def test_the_gaussian_lds_formula_is_the_host_functions(built_lib, dims, acts):
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    assert T.lds_bytes_gaussian(dims, acts) == T.lds_bytes_formula_gaussian(dims, acts)
    t = [(d + 15) // 16 for d in dims]
    pre = sum(t[l + 1] for l, a in enumerate(acts) if a == L.ACT_SWISH)
    assert T.lds_bytes_formula_gaussian(dims, acts) == 4 * (256 * (sum(t) + pre + max(t) + t[-1]) + 1088)
    assert T.lds_bytes_gaussian(dims, acts) == T.lds_bytes(dims, acts) + 1024 * t[-1] <= L.TRAIN_LDS_LIMIT
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4 * (256 * (sum_l T_l + sum over swish layers of T_{l+1} + max_l T_l + T_L) + 1088)" in design
    if dims == (26, 200, 200, 20):
        assert T.lds_bytes_gaussian(dims, acts) == 50432 and "50432" in design


def test_a_carve_over_the_limit_is_refused_before_any_device(built_lib):
    """400-512-512-512 passes 159 KiB only WITH the head's 32 tiles: refused as a Gaussian trainer, while the head-less carve
    is inside the limit.  Bounds outside the rule of bbmpc_set_mlp_logvar_head are BBMPC_E_INVALID, also before any device."""
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    dims, acts = (400, 512, 512, 512), (1, 1, 0)                   # 25 + 3 x 32 resident tiles + 32 of scratch = 153
    plain, gaussian = T.lds_bytes(dims, acts), T.lds_bytes_gaussian(dims, acts)
    assert plain <= L.TRAIN_LDS_LIMIT and gaussian == plain + 32 * 1024 and gaussian > L.TRAIN_LDS_LIMIT
    ws = [np.zeros((i, o), F) for i, o in zip(dims[:-1], dims[1:])]
    bs = [np.zeros((o,), F) for o in dims[1:]]
    with pytest.raises(L.BBMPCError) as ei:
        T.HipGaussianTrainer(ws, bs, acts, logvar_head=(np.zeros((dims[-2], dims[-1]), F), np.zeros((dims[-1],), F), -10.0, 0.5))
    assert ei.value.code == L.E_UNSUPPORTED and "LDS" in str(ei.value) and "log-variance head" in str(ei.value)
    for lo, hi in ((-41.0, 0.5), (-10.0, 40.5), (1.0, 0.5), (float("nan"), 0.5), (-10.0, float("inf"))):
        w2, b2 = U.params((4, 8, 3), seed=0)
        with pytest.raises(L.BBMPCError) as ei:
            T.HipGaussianTrainer(w2, b2, [1, 0], logvar_head=(np.zeros((8, 3), F), np.zeros((3,), F), lo, hi))
        assert ei.value.code == L.E_INVALID and "min_logvar" in str(ei.value), (lo, hi)
