"""The reference semantics of a NaN candidate, on the NumPy oracle alone: for every poison pattern of tests/nonfinite_util.py
and every model the GPU cases use, oracle_np.Evaluator gives float32(-1e6) for the poisoned candidates and the clean run's
bits for every other one -- exactly what nonfinite_util.check asserts of the device.

What this pins besides the rule itself: with the seeds in use no clean reward is NaN or -1e6, and through make_mlp_params
weights one NaN action makes the whole reward sum NaN, not merely a part of it (a NaN that an activation or a reward dropped
would leave a finite, wrong score and the pattern would test nothing)."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import nonfinite_util as NF
from tests.test_gpu_mlp import _q4s_user_reward_np
from tests.test_gpu_mlp_kernel_choice import CASES, CHEETAH, PEND, T3, T4, _case, case_inputs, case_oracle

F = np.float32
N, A = NF.GPU_N, NF.GPU_A
gpu_shape, STEP_NETS, step_inputs = NF.gpu_shape, NF.STEP_NETS, NF.step_inputs


MODELS = [_case("cheetah", CHEETAH, T3, None, H=5), _case("pendulum", PEND, T4, None, H=4),
          _case("cheetah_user_reward", CHEETAH, T3, None, reward="user", H=5)]


def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        key = (tuple(c["dims"]), tuple(c["acts"]), c["reward"], c["H"])
        if key not in seen and not c["step"]:
            seen.add(key)
            out.append(c)
    return out


ROLLOUTS = MODELS + [dict(c, id="case_" + c["id"]) for c in _distinct(CASES)]


def test_patterns_poison_what_they_say():
    seq = np.zeros((N, A, 5, 6), F)
    got = {name: (p, hit) for name, p, hit in NF.patterns(seq)}
    assert list(got) == ["first", "last", "comb", "agent"]
    assert np.isnan(got["first"][0][0, 0, 0, 0]) and np.isnan(got["first"][0]).sum() == 1
    assert np.isnan(got["last"][0][N - 1, A - 1, 4, 5]) and np.isnan(got["last"][0]).sum() == 1
    p, hit = got["comb"]
    assert hit == {(n, 0) for n in range(1, N, 4)} and np.isnan(p).sum() == len(hit) == 9
    assert all(np.isnan(p[n, 0, 2, 5 if i % 2 else 0]) for i, n in enumerate(range(1, N, 4)))
    for q in range(0, N - 3, 4):                          # one poisoned particle in every full quad, clean ones on both sides
        assert sum((n, 0) in hit for n in range(q, q + 4)) == 1
    assert got["agent"][1] == {(17, 1)} and not np.isnan(got["agent"][0][:, 0]).any()
    assert not np.isnan(seq).any()                        # the input is left alone
    assert [n for n, _, _ in NF.patterns(np.zeros((5, 1, 2, 1), F))] == ["first", "last", "comb"]


def test_check_refuses_what_it_should():
    clean = np.arange(12, dtype=F).reshape(6, 2) - F(3.5)
    good = clean.copy()
    good[1, 0] = F(-1e6)
    NF.check(clean, good, {(1, 0)})
    for bad in (clean.copy(),                                              # the rule is missing: the poisoned entry is finite
                np.where(np.arange(12).reshape(6, 2) == 2, F(np.nan), clean).astype(F)):       # ... or NaN
        with pytest.raises(AssertionError):
            NF.check(clean, bad, {(1, 0)})
    leak = good.copy()
    leak[2, 0] = np.nextafter(leak[2, 0], F(10))                           # a neighbour off by one ulp
    with pytest.raises(AssertionError):
        NF.check(clean, leak, {(1, 0)})
    leak = good.copy()
    leak[0, 1] = F(-1e6)                                                   # a neighbour dragged along
    with pytest.raises(AssertionError):
        NF.check(clean, leak, {(1, 0)})
    with pytest.raises(AssertionError):
        NF.check(clean.astype(np.float64), good.astype(np.float64), {(1, 0)})


@pytest.mark.parametrize("case", ROLLOUTS, ids=[c["id"] for c in ROLLOUTS])
def test_oracle_satisfies_check(case):
    c = gpu_shape(case)
    _, _, _, ev = case_oracle(c)
    states, seq = case_inputs(c)
    with np.errstate(all="ignore"):
        clean = ev(states, seq)
        assert np.all(np.isfinite(clean))
        pats = NF.patterns(seq)
        assert len(pats) == 4
        for name, poisoned, hit in pats:
            NF.check(clean, ev(states, poisoned), hit, "%s %s" % (c["id"], name))


@pytest.mark.parametrize("net", STEP_NETS, ids=[n[0] for n in STEP_NETS])
@pytest.mark.parametrize("B", [9, 40])
def test_oracle_one_step_rows_are_independent(net, B):
    c = _case(net[0], net[1], net[2], None)
    _, _, _, ev = case_oracle(c)
    s, a = step_inputs(c, B)
    with np.errstate(all="ignore"):
        nxt = ev.predict_next_state(s, a)
        rew = ev.evaluate_next_reward(s, nxt, a)
        assert np.all(np.isfinite(nxt)) and np.all(np.isfinite(rew))
        for row in (0, B - 1):
            ap = a.copy()
            ap[row, -1] = np.nan
            got = ev.predict_next_state(s, ap)
            assert np.all(np.isnan(got[row]))             # every output of a Dense stack sees every input
            NF.check_rows(nxt, got, got[[row]], [row])
            gr = ev.evaluate_next_reward(s, nxt, ap)
            NF.check_rows(rew, gr, gr[[row]], [row])


def test_user_reward_model_is_the_one_of_the_gpu_cases():
    assert case_oracle(MODELS[2])[3].reward is _q4s_user_reward_np
