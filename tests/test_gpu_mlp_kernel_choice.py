"""Which learned-model rollout kernel Engine::choose_rollout_mlp (csrc/bbmpc_mlp.hip) picks, one case per branch of the
choice: the plain name (bbmpc_get_profile), the instantiation (bbmpc_profile_instantiation) and the rewards against the
float oracle.  tools/mlp_choice_dump.py runs the same table and keeps every result, to compare two builds bit for bit.

Tolerances as tests/test_gpu_mlp.py: H-step rewards rtol 1e-3 + atol 1e-3 * H, a single model step rtol 2e-5 + atol 2e-5;
the opt-in bf16 modes keep the bounds of test_optional_bf16_modes_against_oracle there.

The *_ext instantiations of k_rollout_mlp_w4 are written as "k_rollout_mlp_w4_ext<L>", which bbmpc_profile_instantiation
reports only where it extends the plain name with '<': for them both calls give "k_rollout_mlp_w4"."""
import os

import numpy as np
import pytest

from tests.parity_util import assert_cheetah_rewards, cheetah_threshold_margin
from tests.test_gpu_activations import CODE, MLP64
from tests.test_gpu_mlp import Q4S_USER_REWARD, _problem, _q4s_user_reward_np, _stats

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
F = np.float32
EXT = ("elu", "swish")

CHEETAH = [26, 200, 200, 20]
WIDE = [26, 256, 256, 20]
FULL13 = [26, 208, 208, 20]                     # spec 1 with thirteen full hidden tiles: outside the 200-unit family's kernels
DEEP = [26, 500, 500, 500, 20]
PEND = [4, 32, 32, 32, 3]
T3, T4 = ["tanh", "tanh", None], ["tanh", "tanh", "tanh", None]
BF16_3 = dict(q99=1e-3, big=0.05, frac=0.005, median=2e-4)
BF16_1 = dict(q99=15.0, big=5.0, frac=0.1, median=0.1)


def _case(cid, dims, acts, name, inst=None, env=None, reward=None, N=8, A=1, H=4, bf16=None, step=False):
    S = 3 if dims[0] == 4 else dims[-1]
    return dict(id=cid, dims=dims, acts=acts, S=S, U=dims[0] - S, reward=reward or ("pendulum" if S == 3 else "cheetah"),
                env=env or {}, N=N, A=A, H=H, name=name, inst=inst or name, bf16=bf16, step=step)


CASES = [
    _case("generic_spec0", DEEP, T4, "k_rollout_mlp", H=3),
    _case("generic_spec1", FULL13, ["tanh", "relu", None], "k_rollout_mlp", A=2),
    _case("generic_spec2", PEND, T4, "k_rollout_mlp", env={"BBMPC_MLP_WAVE": "0", "BBMPC_MLP_W4": "0"}, A=2),
    _case("generic_ext_spec0", DEEP, ["tanh", "swish", "tanh", None], "k_rollout_mlp", H=3),
    _case("generic_ext_spec1", FULL13, ["elu", "tanh", None], "k_rollout_mlp"),
    _case("generic_ext_spec2", PEND, ["tanh", "elu", "tanh", None], "k_rollout_mlp", env={"BBMPC_MLP_WAVE": "0", "BBMPC_MLP_W4": "0"}),
    _case("bf16_1", CHEETAH, T3, "k_rollout_mlp_bf16<1>", env={"BBMPC_MLP_BF16": "1"}, H=5, bf16=BF16_1),
    _case("bf16_3", CHEETAH, T3, "k_rollout_mlp_bf16<3>", env={"BBMPC_MLP_BF16": "3"}, H=5, bf16=BF16_3),
    # a HIP-source reward scores the recorded trajectory, which the bf16 kernels do not write
    _case("bf16_3_recording", CHEETAH, T3, "k_rollout_mlp_q4s", "k_rollout_mlp_q4s<50, 7, 1, 1, 0, 1>", env={"BBMPC_MLP_BF16": "3"},
          reward="user", H=5),
    _case("bf16_3_generic", CHEETAH, T3, "k_rollout_mlp", env={"BBMPC_MLP_BF16": "3", "BBMPC_MLP_GENERIC": "1"}, H=5),
    _case("w4_tanh", PEND, T4, "k_rollout_mlp_w4", "k_rollout_mlp_w4<4, true>", A=2),
    _case("w4_relu", PEND, ["relu", "relu", "relu", None], "k_rollout_mlp_w4", "k_rollout_mlp_w4<4, false>"),
    _case("w4_ext", PEND, ["elu", "elu", "elu", None], "k_rollout_mlp_w4"),
    _case("w4_two_layers", [4, 32, 3], ["tanh", None], "k_rollout_mlp_w4", "k_rollout_mlp_w4<2, true>"),
    _case("w4_three_layers", [26, 24, 20, 20], ["sigmoid", "tanh", None], "k_rollout_mlp_w4", "k_rollout_mlp_w4<3, false>"),
    _case("wave_three_tiles", [4, 48, 48, 3], T3, "k_rollout_mlp_wave", A=2),
    _case("wave_ext", [4, 48, 3], ["swish", None], "k_rollout_mlp_wave"),
    _case("wave_w4_off", PEND, T4, "k_rollout_mlp_wave", env={"BBMPC_MLP_W4": "0"}),
    _case("q4s_tanh", CHEETAH, T3, "k_rollout_mlp_q4s", "k_rollout_mlp_q4s<50, 7, 1, 1, 0, 1>", H=5),
    _case("q4s_relu", CHEETAH, ["relu", "relu", None], "k_rollout_mlp_q4s", "k_rollout_mlp_q4s<50, 7, 2, 2, 0, 1>", H=5),
    _case("q4s_mixed", CHEETAH, ["sigmoid", "tanh", None], "k_rollout_mlp_q4s", "k_rollout_mlp_q4s<50, 7, -1, -1, -1, 1>", A=2, H=5),
    _case("q4s_ext", CHEETAH, ["swish", "swish", None], "k_rollout_mlp_q4s", "k_rollout_mlp_q4s<50, 7, -2, -2, -2, 1>", H=5),
    _case("q4s_wide_tanh", WIDE, T3, "k_rollout_mlp_q4s", "k_rollout_mlp_q4s<64, 7, 1, 1, 0, 1>", H=5),
    _case("q4s_wide_relu", WIDE, ["relu", "relu", None], "k_rollout_mlp_q4s", "k_rollout_mlp_q4s<64, 7, -1, -1, -1, 1>", H=5),
    # two action pairs per thread from 4 * ceil(H * U / 4) = 257 on: dim_U = 8 (the kernel's limit) reaches it first, at H = 33
    _case("q4s_two_pairs", [28, 200, 200, 20], T3, "k_rollout_mlp_q4s", "k_rollout_mlp_q4s<50, 7, 1, 1, 0, 2>", H=33),
    _case("q4", CHEETAH, T3, "k_rollout_mlp_q4", env={"BBMPC_MLP_Q4S": "0"}, H=5),
    _case("pair_one_tile", CHEETAH, T3, "k_rollout_mlp_pair", env={"BBMPC_MLP_Q4": "0"}, A=2, H=5),
    _case("pair_two_tiles", CHEETAH, T3, "k_rollout_mlp_pair", env={"BBMPC_MLP_Q4": "0", "BBMPC_MLP_PAIR": "1"}, N=32, H=5),
    _case("pair_two_tiles_h50", CHEETAH, T3, "k_rollout_mlp_pair", env={"BBMPC_MLP_Q4": "0", "BBMPC_MLP_PAIR": "1"}, N=32, H=50),
    _case("pair_two_tiles_h50_recording", CHEETAH, T3, "k_rollout_mlp_pair", env={"BBMPC_MLP_Q4": "0", "BBMPC_MLP_PAIR": "1"},
          reward="user", N=32, H=50),
    _case("pair_two_tiles_other_dims", [24, 200, 200, 19], T3, "k_rollout_mlp_pair", env={"BBMPC_MLP_Q4": "0", "BBMPC_MLP_PAIR": "1"},
          N=32, H=5),
    _case("forced_generic_cheetah", CHEETAH, T3, "k_rollout_mlp", env={"BBMPC_MLP_GENERIC": "1"}, H=5),
    _case("forced_generic_w4_shape", PEND, T4, "k_rollout_mlp", env={"BBMPC_MLP_GENERIC": "1"}),
    # bbmpc_predict_next_state on more than 32 rows: the one-step form, which reports no name
    _case("step", CHEETAH, T3, None, N=40, step=True),
    _case("step_ext", CHEETAH, ["elu", "tanh", None], None, N=40, step=True),
]


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def case_oracle(c, seed=42):
    """-> (weights, biases, stats, oracle evaluator) of a case, without a device: the parameters _problem draws for `seed`"""
    dims, acts, S, U = c["dims"], c["acts"], c["S"], c["U"]
    ws, bs = O.make_mlp_params(dims, seed=seed)
    rng = np.random.default_rng(seed + 1)
    bs = [rng.normal(0, 0.05, b.shape).astype(F) for b in bs]
    stats = _stats(S, U, seed + 2)
    net = MLP64(ws, bs, acts) if any(a in EXT for a in acts) else O.MLP(ws, bs, acts)
    ev = O.Evaluator(_q4s_user_reward_np if c["reward"] == "user" else c["reward"], O.Handler(net, False, True, stats))
    return ws, bs, stats, ev


def case_inputs(c):
    """-> (start states [A, S], action sequences [N, A, H, U]) of a rollout case"""
    rng = np.random.default_rng(sum(c["dims"]) + c["N"] + c["H"])
    states = O.pendulum_start_states(c["A"]) if c["reward"] == "pendulum" else O.cheetah_start_states(c["A"], c["S"])
    return states, rng.uniform(-1, 1, (c["N"], c["A"], c["H"], c["U"])).astype(F)


def build_case(L, c, setenv):
    """-> (engine, oracle evaluator) of a case; setenv(key, value) is called for the case's switches before the engine is
    created (they are read there).  tests/test_gpu_nonfinite_candidates.py builds its engines here too."""
    from blackbox_mpc_amd.engine import Engine
    for k, v in c["env"].items():
        setenv(k, v)
    dims, acts, S, U, A, H = c["dims"], c["acts"], c["S"], c["U"], c["A"], c["H"]
    if c["reward"] == "user" or any(a in EXT for a in acts):
        ws, bs, stats, ev = case_oracle(c)
        rk = {"cheetah": L.REW_CHEETAH, "pendulum": L.REW_PENDULUM, "user": L.REW_USER}[c["reward"]]
        eng = Engine(L.OPT_NONE, L.DYN_MLP, rk, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=A, planning_horizon=H)
        if c["reward"] == "user":
            eng.set_reward_source(Q4S_USER_REWARD)
        eng.set_mlp(ws, bs, [CODE[a] for a in acts], stats)
    else:
        eng, ev, _, _ = _problem(L, dims, acts, S, U, c["reward"], True, seed=42, A=A, H=H)
    return eng, ev


def run_case(L, c, setenv):
    """-> (device result, oracle result, plain name, instantiation, evaluator, states, sequences)"""
    eng, ev = build_case(L, c, setenv)
    dims, S, U, A, H, N = c["dims"], c["S"], c["U"], c["A"], c["H"], c["N"]
    rng = np.random.default_rng(sum(dims) + N + H)
    if c["step"]:
        s = rng.normal(0, 0.5, (N, S)).astype(F)
        a = rng.uniform(-1, 1, (N, U)).astype(F)
        return eng.predict_next_state(s, a), ev.predict_next_state(s, a), None, None, ev, s, a
    states, seq = case_inputs(c)
    got = eng.evaluate(states, seq)
    return got, ev(states, seq), eng.get_profile()[2], eng.profile_instantiation(), ev, states, seq


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernel_choice(L, monkeypatch, case):
    for k in [k for k in os.environ if k.startswith("BBMPC_MLP_")]:
        monkeypatch.delenv(k)
    got, want, name, inst, ev, states, seq = run_case(L, case, monkeypatch.setenv)
    H = case["H"]
    print(case["id"], name, inst, "max |err| %.3e" % float(np.max(np.abs(got - want))))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    if case["step"]:
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5)
        return
    assert name == case["name"]
    assert inst == case["inst"]
    if case["id"] == "bf16_3_recording":
        assert not name.startswith("k_rollout_mlp_bf16")
    if case["bf16"]:
        b, err = case["bf16"], np.abs(got - want)
        assert np.quantile(err, 0.99) < b["q99"]
        assert (err > b["big"]).mean() < b["frac"]
        assert np.median(err) < b["median"]
    elif case["reward"] == "cheetah":
        assert_cheetah_rewards(got, want, 1e-3, 1e-3 * H, margin=lambda: cheetah_threshold_margin(ev, states, seq))
    else:
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)
