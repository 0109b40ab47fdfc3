"""HIP-source rewards for the particle evaluator's tests and their NumPy twins (float32, one rounding per source
operation, the argument order of the call: (current_state, actions, next_state))."""
import numpy as np

from oracle import oracle_np as O

F = np.float32

# reads the action, the current state and the next state, each in a term of its own: a wrong candidate, a swapped argument
# or a stale state shows in the return
MIXED_REWARD = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    const float d = nxt[0] - 0.5f;
    float r = -(d * d);
    r = r - 0.1f * (cur[2] * cur[2]);
    r = r - 0.3f * (act[U - 1] * nxt[1]);
    return r;
}
"""


def mixed_np(cur, act, nxt):
    cur, act, nxt = O.f32(cur), O.f32(act), O.f32(nxt)
    d = (nxt[:, 0] - F(0.5)).astype(F)
    r = (-(d * d)).astype(F)
    r = (r - (F(0.1) * (cur[:, 2] * cur[:, 2]).astype(F)).astype(F)).astype(F)
    r = (r - (F(0.3) * (act[:, -1] * nxt[:, 1]).astype(F)).astype(F)).astype(F)
    return r


def mixed64(cur, act, nxt):
    cur, act, nxt = (np.asarray(v, np.float64) for v in (cur, act, nxt))
    return -(nxt[:, 0] - 0.5) ** 2 - 0.1 * cur[:, 2] ** 2 - 0.3 * act[:, -1] * nxt[:, 1]


# the built-in pendulum reward AS EXECUTED (models.hpp reward_generic, REW_PENDULUM without the Q1 fix: the action term
# squares the next state), operation for operation; atan2f and fmodf stand for the engine's own forms of them
PENDULUM_AS_EXECUTED = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    const float PI = 3.14159274101257324f, TWO_PI = 6.28318548202514648f;
    const float theta = atan2f(cur[1], cur[0]);
    float ss = 0.0f;
    for (int s = 0; s < S; ++s) ss = ss + nxt[s] * nxt[s];
    float m = fmodf(theta + PI, TWO_PI);
    if (m != 0.0f && m < 0.0f) m = m + TWO_PI;
    const float ang = m - PI;
    const float first = ang * ang + 0.1f * (cur[2] * cur[2]);
    return (-first) - 0.001f * ss;
}
"""

# two runtime parameters per agent (a goal for nxt[0], an action weight) and the planning step t
GOAL_STEP_REWARD = """
__device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,
                                          const float* params, int t) {
    const float d = nxt[0] - params[0];
    float r = -(d * d);
    r = r - params[1] * (act[0] * act[0]);
    r = r - (0.05f * (float)t) * (cur[2] * cur[2]);
    return r;
}
"""


def goal_step_np(cur, act, nxt, params, t):
    """params [B, 2]: every row's own parameter row; t: the step."""
    cur, act, nxt, params = O.f32(cur), O.f32(act), O.f32(nxt), O.f32(params)
    d = (nxt[:, 0] - params[:, 0]).astype(F)
    r = (-(d * d)).astype(F)
    r = (r - (params[:, 1] * (act[:, 0] * act[:, 0]).astype(F)).astype(F)).astype(F)
    r = (r - ((F(0.05) * F(t)).astype(F) * (cur[:, 2] * cur[:, 2]).astype(F)).astype(F)).astype(F)
    return r


class GoalStepReward:
    """goal_step_np as the `reward(cur, act, nxt)` callable particle_util.particle_returns wants: its rows are
    b = (n * P + p) * A + a, so row b reads agent b % A's parameters, and it calls the reward once per step, in order."""

    def __init__(self, params):
        self.params = O.f32(params)          # [A, 2]
        self.t = 0

    def __call__(self, cur, act, nxt):
        rows = self.params[np.arange(cur.shape[0]) % self.params.shape[0]]
        r = goal_step_np(cur, act, nxt, rows, self.t)
        self.t += 1
        return r


# NaN exactly where the next state's third component exceeds a threshold
NAN_ABOVE_REWARD = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    if (nxt[2] > 50.0f) return nanf("");
    return -(nxt[0] * nxt[0]) - 0.1f * (act[0] * act[0]);
}
"""
