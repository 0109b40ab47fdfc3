"""What the learned-reward scorer (csrc/kernels_reward_mlp.hpp) costs next to the rollout it follows.  Prints markdown; the
committed copy is profiles/reward_mlp.md.

    python tools/reward_mlp_rate.py > profiles/reward_mlp.md

Method.  Kernel times come from the handle's profiling events (bbmpc_set_profiling, every launch; mean over `reps`
launches) -- the method bench.py's roofline block uses.  They bracket the rollout kernel; a handle created with
BBMPC_PROF_REWARD_MLP=1 in the environment brackets k_reward_mlp_traj instead, so the scorer's kernel is timed on its own
(k_reward_mlp_finish, one lane per candidate adding H floats, is not in it).  The handle runs on a torch stream; one
evaluate_dev (rollout + both scorer kernels + result copies) is also timed with events on that stream, median of `reps`
calls after a warm-up.  FLOPs = 2 * rows * sum(in * out) over the Dense
layers; the peak is bench.py's MFMA_F32_PEAK_TFLOPS."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MFMA_F32_PEAK_TFLOPS = 157.3           # bench.py
F = np.float32


def _params(dims, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0, 1 / np.sqrt(k), (k, m)).astype(F) for k, m in zip(dims[:-1], dims[1:])]
    return ws, [rng.normal(0, 0.05, (m,)).astype(F) for m in dims[1:]]


def _flops(dims, rows):
    return 2.0 * rows * sum(k * m for k, m in zip(dims[:-1], dims[1:]))


def _median_ms(torch, stream, fn, reps, warm=5):
    for _ in range(warm):
        fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def _twin_source(S, U, hidden):
    # the 7-20-1 tanh network as HIP source with its weights as runtime parameters (the layout of tests/reward_mlp_util.py)
    D = 2 * S + U
    return """
__device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U, const float* p, int t) {
    float x[%(D)d];
    int k = 0;
    for (int i = 0; i < %(S)d; ++i) x[k++] = cur[i];
    for (int i = 0; i < %(U)d; ++i) x[k++] = act[i];
    for (int i = 0; i < %(S)d; ++i) x[k++] = nxt[i];
    float y = p[%(ob)d];
    for (int j = 0; j < %(Hd)d; ++j) {
        float v = p[%(b0)d + j];
        for (int i = 0; i < %(D)d; ++i) v = v + x[i] * p[i * %(Hd)d + j];
        y = y + tanhf(v) * p[%(w1)d + j];
    }
    return y;
}
""" % dict(D=D, S=S, U=U, Hd=hidden, b0=D * hidden, w1=D * hidden + hidden, ob=D * hidden + 2 * hidden)


def main(reps=50):
    import torch
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.engine import Engine
    stream = torch.cuda.Stream()
    lines = ["# Learned reward scorer: measured cost", "",
             "Produced by `tools/reward_mlp_rate.py` on %s; every figure below comes from this one build."
             % torch.cuda.get_device_name(0), ""]

    def handle(S, U, H, dyn_dims, reward, opt=L.OPT_NONE, prof_scorer=False, **kw):
        if prof_scorer:
            os.environ["BBMPC_PROF_REWARD_MLP"] = "1"          # read once, when the handle is created
        try:
            eng = Engine(opt, L.DYN_MLP, reward, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=1, planning_horizon=H, **kw)
        finally:
            os.environ.pop("BBMPC_PROF_REWARD_MLP", None)
        ws, bs = _params(dyn_dims, 1)
        ws[-1] *= F(0.05)
        eng.set_mlp(ws, bs, [L.ACT_TANH] * (len(ws) - 1) + [L.ACT_NONE], None)
        eng.set_torch_stream(stream)
        return eng

    def evaluate_times(eng, S, U, N, H):
        """(evaluate_dev by stream events, the bracketed kernel by profiling events, its name), ms"""
        st = torch.zeros((1, S), device="cuda") + 0.1
        seq = (torch.rand((N, 1, H, U), device="cuda") * 2 - 1).contiguous()
        out = torch.empty((N, 1), device="cuda")
        torch.cuda.synchronize()
        fn = lambda: eng.evaluate_dev(st.data_ptr(), seq.data_ptr(), N, out.data_ptr())
        total = _median_ms(torch, stream, fn, reps)
        eng.set_profiling(True)
        eng.get_profile()
        for _ in range(reps):
            fn()
        stream.synchronize()
        ms, n, name = eng.get_profile()
        eng.set_profiling(False)
        return total, ms / max(n, 1), name

    def row(what, ms, flops):
        return "| %s | %.1f | %.2f | %.2f | %.1f %% |" % (what, ms * 1e3, flops / 1e9, flops / ms / 1e9, 100 * flops / ms / 1e9 / MFMA_F32_PEAK_TFLOPS)

    # ---- the flagship shape ------------------------------------------------------------------------------------------
    S, U, N, H = 20, 6, 1000, 30
    dyn, rew = [26, 200, 200, 20], [46, 200, 200, 1]
    acts = [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE]
    rw, rb = _params(rew, 2)
    eng = handle(S, U, H, dyn, L.REW_MLP)
    eng.set_reward_mlp(rw, rb, acts, 7, None)
    total, roll, name = evaluate_times(eng, S, U, N, H)
    eng_s = handle(S, U, H, dyn, L.REW_MLP, prof_scorer=True)
    eng_s.set_reward_mlp(rw, rb, acts, 7, None)
    _, scorer, sname = evaluate_times(eng_s, S, U, N, H)
    fl_s, fl_r = _flops(rew, N * H), _flops(dyn, N * H)
    lines += ["## N = 1000, H = 30, S = 20, U = 6; dynamics 26-200-200-20, reward network 46-200-200-1", "",
              "| quantity | time [us] | GFLOP | TFLOP/s | of the fp32-MFMA peak (%.1f) |" % MFMA_F32_PEAK_TFLOPS, "|---|---|---|---|---|",
              row("scorer kernel `%s` (profiling events)" % sname, scorer, fl_s),
              row("rollout kernel `%s`, reward kind REW_NONE, trajectory recorded (profiling events)" % name, roll, fl_r),
              "| evaluate_dev, REW_MLP: rollout + k_reward_mlp_traj + k_reward_mlp_finish + result copy (stream events) | %.1f | | | |" % (total * 1e3),
              ""]
    lines += ["The scorer kernel %s the rollout kernel it follows (%.1f us against %.1f us)." %
              ("takes no longer than" if scorer <= roll else "TAKES LONGER THAN", scorer * 1e3, roll * 1e3), ""]

    # ---- a five-iteration CEM control step: REW_MLP against REW_CHEETAH on the same model ---------------------------------
    res = {}
    for label, kind in (("REW_MLP", L.REW_MLP), ("REW_CHEETAH", L.REW_CHEETAH)):
        e = handle(S, U, H, dyn, kind, opt=L.OPT_CEM, population_size=N, max_iterations=5, num_elite=50, seed=1)
        if kind == L.REW_MLP:
            e.set_reward_mlp(rw, rb, acts, 7, None)
        st = torch.zeros((1, S), device="cuda") + 0.1
        rec = torch.empty((1, U + S + 1), device="cuda")
        torch.cuda.synchronize()
        res[label] = _median_ms(torch, stream, lambda: e.optimize_dev(st.data_ptr(), rec.data_ptr()), reps)
    lines += ["## CEM control step, 5 iterations, N = 1000, H = 30 (optimize_dev, stream events)", "",
              "| reward | time per control step [us] |", "|---|---|",
              "| REW_MLP (launch sequence per iteration: rollout, scorer, finish, refit) | %.1f |" % (res["REW_MLP"] * 1e3),
              "| REW_CHEETAH (built-in reward inside the rollout kernel; the handle's usual launch sequence) | %.1f |" % (res["REW_CHEETAH"] * 1e3), ""]

    # ---- the small shape against the HIP-source twin -----------------------------------------------------------------------
    S, U, N, H = 3, 1, 500, 30
    dyn, rew = [4, 24, 3], [7, 20, 1]
    rw, rb = _params(rew, 3)
    a = handle(S, U, H, dyn, L.REW_MLP)
    a.set_reward_mlp(rw, rb, [L.ACT_TANH, L.ACT_NONE], 7, None)
    a_s = handle(S, U, H, dyn, L.REW_MLP, prof_scorer=True)
    a_s.set_reward_mlp(rw, rb, [L.ACT_TANH, L.ACT_NONE], 7, None)
    b = handle(S, U, H, dyn, L.REW_USER)
    params = np.concatenate([rw[0].reshape(-1), rb[0], rw[1].reshape(-1), rb[1]]).astype(F)
    b.set_reward_source(_twin_source(S, U, 20), params.size)
    b.set_user_params(L.USER_KIND_REWARD, params)
    ta, ra, _ = evaluate_times(a, S, U, N, H)
    _, sa, _ = evaluate_times(a_s, S, U, N, H)
    tb, rbk, _ = evaluate_times(b, S, U, N, H)
    lines += ["## N = 500, H = 30, S = 3, U = 1; reward network 7-20-1 against its HIP-source twin", "",
              "The twin's scorer kernel is compiled at run time and has no profiling bracket: both handles are compared on what",
              "evaluate_dev takes beyond the rollout kernel (scorer kernels + launch gaps + result copy).", "",
              "| handle | evaluate_dev [us] | rollout kernel [us] | beyond the rollout kernel [us] | k_reward_mlp_traj alone [us] |", "|---|---|---|---|---|",
              "| REW_MLP (k_reward_mlp_traj + k_reward_mlp_finish) | %.1f | %.1f | %.1f | %.1f |" % (ta * 1e3, ra * 1e3, (ta - ra) * 1e3, sa * 1e3),
              "| REW_USER, HIP source with 181 runtime parameters (bbmpc_user_reward_traj, one lane per candidate) | %.1f | %.1f | %.1f | |"
              % (tb * 1e3, rbk * 1e3, (tb - rbk) * 1e3), ""]
    print("\n".join(lines))


if __name__ == "__main__":
    main()
