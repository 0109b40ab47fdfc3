"""Measurements behind profiles/correlated_sampling.md: run on an MI355X with the library built,

    python tools/correlated_sampling.py [OUT_DIR]            # writes OUT_DIR/correlated_sampling.md (default profiles/)

1. kernel time of k_gen_candidates_corr next to k_gen_candidates<SRC_TRUNC> (rocprofv3 --kernel-trace around a child
   process running `--kernels`), at N=500, H=30, U=1 (pendulum) and N=1000, H=30, U=6 (26-200-200-20 model);
2. control-step time with and without a mixing matrix on the same route (per-iteration launches with the trace on);
3. closed-loop pendulum return over a fixed set of start states for beta in {0, 1, 2}, CEM N=64, 3 iterations.
"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("BBMPC_FUSED", "0")        # the pendulum's per-iteration kernels: the route a mixing matrix takes
F = np.float32
H = 30
USER_REWARD = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    const float th = atan2f(cur[1], cur[0]);
    return -(th * th + 0.1f * cur[2] * cur[2]) - 0.001f * act[0] * act[0];
}
"""


def _pendulum(L, N, A=1, iters=5, k=50, reward=None, seed=0):
    from blackbox_mpc_amd.engine import Engine
    eng = Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_USER if reward else L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A,
                 planning_horizon=H, population_size=N, max_iterations=iters, num_elite=k, seed=seed)
    if reward:
        eng.set_reward_source(reward)
    return eng


def _cheetah(L, N, iters=5, k=50):
    from blackbox_mpc_amd.engine import Engine
    from oracle import oracle_np as O
    S, U = 20, 6
    ws, bs = O.make_mlp_params([S + U, 200, 200, S], seed=42)
    eng = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_CHEETAH, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=1, planning_horizon=H,
                 population_size=N, max_iterations=iters, num_elite=k)
    eng.set_mlp(ws, bs, [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE], None)
    return eng, O.cheetah_start_states(1, S).astype(F)


def kernels_workload():
    """what the profiler watches: both draw kernels at both shapes, 50 control steps of 5 iterations each"""
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.utils.colored_noise import colored_noise_mixing
    from oracle import oracle_np as O
    M = colored_noise_mixing(H, 2.0)
    s1 = O.pendulum_start_states(1)
    for corr in (False, True):
        eng = _pendulum(L, 500, reward=USER_REWARD)          # a HIP-source reward draws through k_gen_candidates<SRC_TRUNC>
        if corr:
            eng.set_sampling_correlation(M)
        for t in range(50):
            eng.optimize(s1, t)
        eng, s6 = _cheetah(L, 1000)
        if corr:
            eng.set_sampling_correlation(M)
        else:
            eng.set_particles(1, np.zeros(20, F), 0.0)       # the particle evaluator draws through k_gen_candidates<SRC_TRUNC>
        for t in range(50):
            eng.optimize(s6, t)


def kernel_times(out_dir):
    prof = os.path.join(out_dir, "corr_prof")
    shutil.rmtree(prof, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", prof, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--kernels"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    files = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
    if res.returncode != 0 or not files:
        return ["rocprofv3 run failed (exit %d): no kernel times.\n```\n%s\n```" % (res.returncode, (res.stdout + res.stderr)[-1500:])]
    # per (kernel, grid size): the two shapes launch grids of different sizes
    rows = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if "k_gen_candidates" not in name:
            continue
        kind = "k_gen_candidates_corr" if "k_gen_candidates_corr" in name else "k_gen_candidates<SRC_TRUNC>"
        grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r.get("Grid_Size", 0))
        shape = "N=500, H=30, U=1" if grid <= 512 else "N=1000, H=30, U=6"
        rows.setdefault((shape, kind), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    shutil.rmtree(prof, ignore_errors=True)
    lines = ["| shape | kernel | launches | median us | mean us | min us |", "|---|---|---|---|---|---|"]
    for (shape, kind), v in sorted(rows.items()):
        v = np.asarray(v[len(v) // 5:])                      # the first fifth: warm-up
        lines.append("| %s | %s | %d | %.2f | %.2f | %.2f |" % (shape, kind, len(v), np.median(v), v.mean(), v.min()))
    return lines


def step_times():
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.utils.colored_noise import colored_noise_mixing
    from oracle import oracle_np as O
    M = colored_noise_mixing(H, 2.0)
    lines = ["| workload | matrix | us per control step (median of 5 windows of 100 calls) |", "|---|---|---|"]
    for label in ("pendulum CEM N=500 H=30 U=1, 5 iterations", "26-200-200-20 model CEM N=1000 H=30 U=6, 5 iterations"):
        for corr in (False, True):
            if label.startswith("pendulum"):
                eng, s = _pendulum(L, 500), O.pendulum_start_states(1)
            else:
                eng, s = _cheetah(L, 1000)
            eng.set_trace(True)                              # both sides on the per-iteration route
            if corr:
                eng.set_sampling_correlation(M)
            for t in range(30):
                eng.optimize(s, t)
            win = []
            for w in range(5):
                t0 = time.perf_counter()
                for t in range(100):
                    eng.optimize(s, t)
                win.append((time.perf_counter() - t0) / 100 * 1e6)
            lines.append("| %s | %s | %.1f |" % (label, "colored_noise_mixing(30, 2.0)" if corr else "none", np.median(win)))
            eng.close()
    return lines


def closed_loop():
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.utils.colored_noise import colored_noise_mixing
    A, T, seeds = 16, 200, (0, 1, 2)
    th = np.pi - 2.0 * np.pi * np.arange(A) / A                  # 16 start angles around the circle, hanging down first, at rest
    start = np.stack([np.cos(th), np.sin(th), np.zeros(A)], axis=1).astype(F)
    lines = ["| sampling | mean return | std over (start, seed) | worst | upright at the end |", "|---|---|---|---|---|"]
    for label, beta in (("white (no matrix)", None), ("beta = 0 (identity installed)", 0.0), ("beta = 1", 1.0), ("beta = 2", 2.0)):
        rets, up = [], 0
        for seed in seeds:
            eng = _pendulum(L, 64, A=A, iters=3, k=8, seed=seed)
            if beta is not None:
                eng.set_sampling_correlation(colored_noise_mixing(H, beta))
            s, total = start, np.zeros(A)
            for t in range(T):
                _, s, r = eng.optimize(s, t)
                total += r
            rets.append(total)
            up += int(np.sum(s[:, 0] > 0.95))
            eng.close()
        rets = np.concatenate(rets)
        lines.append("| %s | %.1f | %.1f | %.1f | %d / %d |" % (label, rets.mean(), rets.std(), rets.min(), up, A * len(seeds)))
    return lines


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    doc = ["# Temporally correlated sampling: measurements", "",
           "Produced by `python tools/correlated_sampling.py` on one MI355X (DESIGN.md section 8g).  The matrix is",
           "`colored_noise_mixing(30, 2.0)` (lower-triangular: the kernel sums t + 1 terms for row t) unless stated.", "",
           "## Draw kernels (rocprofv3 kernel trace, 250 launches per row, first fifth dropped)", ""]
    doc += kernel_times(out_dir)                                 # first: the profiled child runs before this process opens the GPU
    doc += ["", "## Control step, host in / host out, per-iteration launches with the trace on (`BBMPC_FUSED=0`)", ""]
    doc += step_times()
    doc += ["", "## Closed-loop pendulum, CEM N=64, 8 elites, 3 iterations, H=30, 200 control steps, model = environment", "",
            "16 start angles evenly spaced around the circle (at rest) x 3 seeds; return = sum of the 200 step rewards.", ""]
    doc += closed_loop()
    path = os.path.join(out_dir, "correlated_sampling.md")
    with open(path, "w") as f:
        f.write("\n".join(doc) + "\n")
    print("\n".join(doc))


if __name__ == "__main__":
    if "--kernels" in sys.argv:
        kernels_workload()
    else:
        main()
