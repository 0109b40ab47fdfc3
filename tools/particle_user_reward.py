"""Measurements behind profiles/particle_user_reward.md: run on an MI355X with the library built,

    python tools/particle_user_reward.py [OUT_DIR]      # writes OUT_DIR/particle_user_reward_measured.md (default profiles/)

1. kernel times (rocprofv3 --kernel-trace around a child process running `--kernels`, a run of its own) of the TRAJ form
   of the particle rollout, of the scorer and of the aggregate on a handle whose reward is the cheetah reward restated
   as HIP source, next to the built-in-reward rollout of the same shapes: the 26-200-200-20 model at N 1000, P 4, H 30
   (profiles/particle_rollout.md's shape), a 2-member ensemble and a log-variance head at the same shape;
2. the control-step time of CEM (5 iterations) with the restated reward against the built-in reward, two handles on the
   same weights, in alternating windows.
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
F = np.float32
S, U, H, N, P = 20, 6, 30, 1000, 4
SHAPES = ("plain", "ensemble E=2", "log-variance head")

CHEETAH_SOURCE = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    float r = 0.0f;
    if (cur[5] >= 0.2f) r = r + (-10.0f);
    if (cur[6] >= 0.0f) r = r + (-10.0f);
    if (cur[7] >= 0.0f) r = r + (-10.0f);
    r = r + (nxt[17] - cur[17]) / 0.01f;
    float ss = 0.0f;
    for (int u = 0; u < U; ++u) ss = ss + act[u] * act[u];
    return r - 0.0f * ss;
}
"""


def _handle(L, user, shape, opt=None, iters=0, k=0):
    from blackbox_mpc_amd.engine import Engine
    from oracle import oracle_np as O
    dims = [S + U, 200, 200, S]
    members = [O.make_mlp_params(dims, seed=42 + 10 * e) for e in range(2)]
    eng = Engine(opt if opt is not None else L.OPT_NONE, L.DYN_MLP, L.REW_USER if user else L.REW_CHEETAH, [-1.0] * U, [1.0] * U,
                 dim_s=S, num_agents=1, planning_horizon=H, population_size=N if opt is not None else 0, max_iterations=iters,
                 num_elite=k)
    eng.set_mlp(members[0][0], members[0][1], [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE], None)
    if user:
        eng.set_reward_source(CHEETAH_SOURCE)
    eng.set_particles(P, np.full(S, 0.02, F), 0.0)
    if shape == SHAPES[1]:
        eng.set_mlp_ensemble(members)
    if shape == SHAPES[2]:
        rng = np.random.default_rng(5)
        lim = np.sqrt(6.0 / (200 + S))
        eng.set_mlp_logvar_head([(rng.uniform(-lim, lim, (200, S)).astype(F), rng.normal(-6.0, 1.5, S).astype(F))],
                                np.full(S, -8.0, F), np.full(S, -3.0, F))
    return eng, O.cheetah_start_states(1, S).astype(F)


def kernels_workload():
    """what the profiler watches: 40 bbmpc_evaluate_particles calls per (shape, reward route)"""
    from blackbox_mpc_amd import _lib as L
    seq = np.random.default_rng(1).uniform(-1, 1, (N, 1, H, U)).astype(F)
    for shape in SHAPES:
        for user in (False, True):
            eng, s = _handle(L, user, shape)
            for _ in range(40):
                eng.evaluate_particles(s, seq, want_returns=False)
            eng.close()


def kernel_times(out_dir):
    prof = os.path.join(out_dir, "pur_prof")
    shutil.rmtree(prof, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", prof, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--kernels"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    files = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
    if res.returncode != 0 or not files:
        return ["rocprofv3 run failed (exit %d): no kernel times.\n```\n%s\n```" % (res.returncode, (res.stdout + res.stderr)[-1500:])]
    rows = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if not any(w in name for w in ("k_rollout_mlp_particles_kind", "bbmpc_user_reward_particles", "k_particle_aggregate")):
            continue
        rows.setdefault(name.replace("bbmpc::", "").replace("void ", ""), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    shutil.rmtree(prof, ignore_errors=True)
    lines = ["| kernel (the third template argument true: the TRAJ form) | launches | median us | p10 / p90 us |", "|---|---|---|---|"]
    for name, v in sorted(rows.items()):
        # 40 launches per handle, handles in the workload's order; the first third of every 40 is warm-up
        v = np.asarray(v)
        keep = np.concatenate([v[i + 13:i + 40] for i in range(0, len(v), 40)]) if len(v) % 40 == 0 else v[len(v) // 3:]
        lines.append("| `%s` | %d | %.1f | %.1f / %.1f |" % (name[:110], len(v), np.median(keep), np.percentile(keep, 10), np.percentile(keep, 90)))
    return lines


def step_times():
    from blackbox_mpc_amd import _lib as L
    lines = ["| shape | built-in reward, us | HIP-source reward, us | difference, us | windows built-in (min - max) | windows source (min - max) |",
             "|---|---|---|---|---|---|"]
    for shape in SHAPES:
        arms = {user: _handle(L, user, shape, opt=L.OPT_CEM, iters=5, k=50) for user in (False, True)}
        win = {False: [], True: []}
        for w in range(6):                                   # alternating windows; window 0 warms both arms up
            for user in (False, True):
                eng, s = arms[user]
                for t in range(5):
                    eng.optimize(s, t)
                eng.synchronize()
                t0 = time.perf_counter()
                for t in range(40):
                    eng.optimize(s, t)                       # host in / host out: every call ends in a device synchronise
                if w:
                    win[user].append((time.perf_counter() - t0) / 40 * 1e6)
        b, u = np.asarray(win[False]), np.asarray(win[True])
        lines.append("| %s | %.1f | %.1f | %+.1f | %.1f - %.1f | %.1f - %.1f |" % (
            shape, np.median(b), np.median(u), np.median(u) - np.median(b), b.min(), b.max(), u.min(), u.max()))
        for eng, _ in arms.values():
            eng.close()
    return lines


def main():
    if "--kernels" in sys.argv:
        kernels_workload()
        return
    out_dir = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    text = ["## Kernel times: 26-200-200-20 model, N %d, P %d, H %d, one agent (store traffic of the TRAJ form: rows * H * S * 4 = %.1f MB per launch)"
            % (N, P, H, N * P * H * S * 4 / 1e6), ""]
    text += kernel_times(out_dir)
    text += ["", "## CEM control step (5 iterations, N %d, 50 elites), per-iteration route, median of 5 windows of 40 steps" % N, ""]
    text += step_times()
    path = os.path.join(out_dir, "particle_user_reward_measured.md")
    with open(path, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
