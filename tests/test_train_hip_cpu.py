"""The HIP training backend without a GPU: the tile decomposition the kernels use is the oracle's gradient, every `train`
takes and checks `backend`, log-variance models are refused by name, the C ABI declares and binds the trainer, and the LDS
formula of the documents is the host function's."""
import os
import re

import numpy as np
import pytest

from oracle import oracle_train as OT
from tests import train_hip_util as U
from tests.test_train_cpu import _episodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TRAINER_SYMBOLS = ["bbmpc_trainer_create", "bbmpc_trainer_destroy", "bbmpc_trainer_lds_bytes", "bbmpc_trainer_set_data",
                   "bbmpc_trainer_fit", "bbmpc_trainer_get_params", "bbmpc_trainer_residual_rms", "bbmpc_trainer_gradients"]


@pytest.mark.parametrize("B", [16, 24, 40])
def test_tile_decomposition_is_the_oracle_gradient(B):
    dims, acts = (7, 20, 33, 3), ["tanh", "relu", None]
    ws, bs = U.params(dims, seed=1)
    x, y = U.dataset(B, 7, 3, seed=2)
    loss, gw, gb = U.tile_decomposition(ws, bs, acts, x, y)
    w64, b64 = [w.astype(np.float64) for w in ws], [b.astype(np.float64) for b in bs]
    want_loss, ww, wb = OT.mse_and_grads(w64, b64, acts, x.astype(np.float64), y.astype(np.float64))
    assert abs(loss - want_loss) <= 1e-12
    for got, want in zip(gw + gb, ww + wb):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_rows_past_the_batch_contribute_zeros():
    dims, acts = (7, 20, 3), ["sigmoid", None]                 # sigmoid: a zero row does not give a zero activation
    ws, bs = U.params(dims, seed=3)
    x, y = U.dataset(24, 7, 3, seed=4)
    a = U.tile_decomposition(ws, bs, acts, x, y)
    b = U.mse_and_grads(ws, bs, acts, x, y)
    for got, want in zip(a[1] + a[2], b[1] + b[2]):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def _models():
    from blackbox_mpc_amd.policy_functions.learned_policy_mlp import LearnedPolicyMLP
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP
    from blackbox_mpc_amd.value_functions.learned_value_mlp import LearnedValueMLP
    acts = ["tanh", None]
    return LearnedRewardMLP(3, 1, [8, 1], acts, seed=0), LearnedValueMLP(3, [8, 1], acts, seed=0), LearnedPolicyMLP(3, 1, [8, 1], acts, seed=0)


def _handler(fn):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    return SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn)


def test_an_unknown_backend_is_a_value_error_everywhere(built_lib):
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    from blackbox_mpc_amd.policies import RandomPolicy
    from blackbox_mpc_amd.utils.dynamics_learning import learn_dynamics_from_policy
    obs, acs, rews = _episodes(1, 10, 2, 0)
    for fn in (DeterministicMLP([4, 8, 3], ["tanh", None], seed=0), EnsembleMLP([4, 8, 3], ["tanh", None], num_members=2, seed=0)):
        with pytest.raises(ValueError, match="bogus"):
            _handler(fn).train(obs, acs, rews, epochs=1, batch_size=8, device="cpu", backend="bogus")
    rng = np.random.default_rng(0)
    s, a, s2, r = rng.normal(size=(20, 3)), rng.normal(size=(20, 1)), rng.normal(size=(20, 3)), rng.normal(size=(20,))
    rew, val, pol = _models()
    with pytest.raises(ValueError, match="bogus"):
        rew.train(s, a, s2, r, epochs=1, device="cpu", backend="bogus")
    with pytest.raises(ValueError, match="bogus"):
        val.train(s, r, epochs=1, device="cpu", backend="bogus")
    with pytest.raises(ValueError, match="bogus"):
        val.train_on_rollouts(obs, rews, 2, epochs=1, device="cpu", backend="bogus")
    with pytest.raises(ValueError, match="bogus"):
        pol.train(s, a, epochs=1, device="cpu", backend="bogus")
    with pytest.raises(ValueError, match="bogus"):
        pol.train_on_rollouts(obs, acs, epochs=1, device="cpu", backend="bogus")

    class _Env:                                                # the rollouts happen before the fit: a two-step stand-in
        from blackbox_mpc_amd import Box
        action_space, observation_space = Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8])

        def reset(self):
            return np.zeros((2, 3), F)

        def step(self, action):
            return np.zeros((2, 3), F), np.zeros((2,), F), False, {}

    with pytest.raises(ValueError, match="bogus"):
        learn_dynamics_from_policy(_Env(), RandomPolicy(2, _Env.action_space, seed=0), 1, 4,
                                   dynamics_function=DeterministicMLP([4, 8, 3], ["tanh", None], seed=0), epochs=1,
                                   batch_size=4, device="cpu", backend="bogus")


def test_the_default_backend_is_torch_and_still_trains_on_the_host(built_lib):
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    obs, acs, rews = _episodes(1, 20, 2, 0)
    h = _handler(DeterministicMLP([4, 8, 3], ["tanh", None], seed=0))
    h.train(obs, acs, rews, epochs=1, batch_size=8, device="cpu", seed=0)
    assert np.isfinite(h.training_loss[0])


def test_log_variance_models_are_refused_by_name(built_lib):
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
    with pytest.raises(ValueError, match="backend='torch'"):
        HipDenseTrainer(ws, bs, [1, 0], device="cpu")


def test_the_trainer_is_declared_and_bound(built_lib):
    import ctypes
    from blackbox_mpc_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)             # entry points added, no struct changed
    assert "typedef struct bbmpc_trainer_s* bbmpc_trainer;" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(built_lib)
    for name in TRAINER_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(L.lib, name).argtypes is not None, name
    for rule, value in (("ADAM", L.TRAIN_ADAM), ("SGD", L.TRAIN_SGD), ("RMSPROP", L.TRAIN_RMSPROP)):
        assert re.search(r"#define\s+BBMPC_TRAIN_%s\s+%d\b" % (rule, value), text)
    src = open(os.path.join(ROOT, "blackbox_mpc_amd", "_build.py")).read()
    assert '"bbmpc_train.hip"' in src


def test_refusals_come_before_any_device(built_lib):
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer
    for dims, acts, code in [((4,) + (8,) * 8 + (3,), [1] * 9, L.E_UNSUPPORTED), ((4, 513, 3), [1, 0], L.E_UNSUPPORTED),
                             ((512,) * 9, [1] * 8, L.E_UNSUPPORTED), ((4, 8, 3), [13, 0], L.E_INVALID)]:
        ws = [np.zeros((i, o), F) for i, o in zip(dims[:-1], dims[1:])]
        bs = [np.zeros((o,), F) for o in dims[1:]]
        with pytest.raises(L.BBMPCError) as ei:
            HipDenseTrainer(ws, bs, acts)
        assert ei.value.code == code and "trainer" in str(ei.value)
    assert L.lib.bbmpc_trainer_destroy(None) == 0


@pytest.mark.parametrize("dims,acts", [((26, 200, 200, 20), (1, 1, 0)), ((512,) * 9, (1,) * 8), ((7, 20, 33, 1), (10, 1, 0)),
                                       ((26, 500, 500, 500, 20), (1, 1, 1, 0))])
def test_the_documented_lds_formula_is_the_host_functions(built_lib, dims, acts):
    from blackbox_mpc_amd.dynamics_functions._train_hip import lds_bytes, lds_bytes_formula
    assert lds_bytes(dims, acts) == lds_bytes_formula(dims, acts)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4 * (256 * (sum_l T_l + sum over swish layers of T_{l+1} + max_l T_l) + 1088)" in design
    if dims == (26, 200, 200, 20):
        assert lds_bytes(dims, acts) == 48384 and "48384" in design
    if dims == (512,) * 9:
        assert lds_bytes(dims, acts) == 332032 > 159 * 1024 and "332032" in design


def test_the_permutation_generator_is_a_permutation():
    from blackbox_mpc_amd.dynamics_functions._train_hip import draw_permutation
    p = draw_permutation(7, 0, 100)
    assert sorted(p.tolist()) == list(range(100))
    assert not np.array_equal(p, draw_permutation(7, 1, 100)) and np.array_equal(p, draw_permutation(7, 0, 100))
