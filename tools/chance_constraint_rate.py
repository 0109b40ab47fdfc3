"""Measurements behind profiles/chance_constraint.md: run on an MI355X with the library built,

    python tools/chance_constraint_rate.py [OUT_DIR]      # writes OUT_DIR/chance_constraint.md (default profiles/)

The 26-200-200-20 cheetah model, N 500, P 20, H 30, one agent, four handles on the same weights: the built-in cheetah
reward and the same reward restated as HIP source, each without and with a chance constraint (an upper bound on one
feature, weight 0 so that the plans do not move).
1. kernel times (rocprofv3 --kernel-trace around a child process running `--kernels`, a run of its own) of the particle
   rollout, the box scan, the user scorer, the aggregate and the apply kernel;
2. one rollout_particles (bbmpc_evaluate_particles without the returns) and a control step of PI2 and CEM (3 iterations),
   constraint on against off, in alternating windows; the off arm is measured twice so that its own spread is on the page.
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
S, U, H, N, P = 20, 6, 30, 500, 20
ITERS = 3

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


def _handle(L, user, constrained, opt=None):
    from blackbox_mpc_amd.engine import Engine
    from oracle import oracle_np as O
    ws, bs = O.make_mlp_params([S + U, 200, 200, S], seed=42)
    eng = Engine(opt if opt is not None else L.OPT_NONE, L.DYN_MLP, L.REW_USER if user else L.REW_CHEETAH, [-1.0] * U, [1.0] * U,
                 dim_s=S, num_agents=1, planning_horizon=H, population_size=N if opt is not None else 0,
                 max_iterations=ITERS if opt is not None else 0, num_elite=50 if opt is not None else 0)
    eng.set_mlp(ws, bs, [L.ACT_TANH, L.ACT_TANH, L.ACT_NONE], None)
    if user:
        eng.set_reward_source(CHEETAH_SOURCE)
    eng.set_particles(P, np.full(S, 0.02, F), 0.0)
    if constrained:
        hi = np.full(S, np.inf, F)
        hi[8] = 0.5
        eng.set_chance_constraint(np.full(S, -np.inf, F), hi, 0.1, 0.0)
    return eng, O.cheetah_start_states(1, S).astype(F)


ARMS = [("built-in reward", False, False), ("built-in reward + constraint", False, True),
        ("HIP-source reward", True, False), ("HIP-source reward + constraint", True, True)]


def kernels_workload():
    """what the profiler watches: 40 bbmpc_evaluate_particles calls per arm"""
    from blackbox_mpc_amd import _lib as L
    seq = np.random.default_rng(1).uniform(-1, 1, (N, 1, H, U)).astype(F)
    for _, user, constrained in ARMS:
        eng, s = _handle(L, user, constrained)
        for _ in range(40):
            eng.evaluate_particles(s, seq, want_returns=False)
        eng.close()


def kernel_times(out_dir):
    prof = os.path.join(out_dir, "cc_prof")
    shutil.rmtree(prof, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", prof, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--kernels"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    files = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
    if res.returncode != 0 or not files:
        return ["rocprofv3 run failed (exit %d): no kernel times.\n```\n%s\n```" % (res.returncode, (res.stdout + res.stderr)[-1500:])]
    rows = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if not any(w in name for w in ("k_rollout_mlp_particles_kind", "bbmpc_user_reward_particles", "k_particle_aggregate",
                                       "k_particle_box_scan", "k_particle_constraint_apply")):
            continue
        rows.setdefault(name.replace("bbmpc::", "").replace("void ", ""), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    shutil.rmtree(prof, ignore_errors=True)
    lines = ["| kernel (rollout: the third template argument true is the TRAJ form; scan: true is box-and-reward) | launches | median us | p10 / p90 us |",
             "|---|---|---|---|"]
    for name, v in sorted(rows.items()):
        v = np.asarray(v)                                   # 40 launches per handle; the first third of every 40 is warm-up
        keep = np.concatenate([v[i + 13:i + 40] for i in range(0, len(v), 40)]) if len(v) % 40 == 0 else v[len(v) // 3:]
        lines.append("| `%s` | %d | %.1f | %.1f / %.1f |" % (name[:120], len(v), np.median(keep), np.percentile(keep, 10), np.percentile(keep, 90)))
    return lines


def _windows(arms, call, reps):
    """alternating windows over the arms; window 0 warms every arm up.  -> {arm: [us per call]}"""
    win = {name: [] for name in arms}
    for w in range(6):
        for name, (eng, s) in arms.items():
            for t in range(3):
                call(eng, s, t)
            eng.synchronize()
            t0 = time.perf_counter()
            for t in range(reps):
                call(eng, s, t)                             # host in / host out: every call ends in a device synchronise
            if w:
                win[name].append((time.perf_counter() - t0) / reps * 1e6)
    return {k: np.asarray(v) for k, v in win.items()}


def _table(title, win):
    lines = ["| %s | median us | windows (min - max) | against its `off` arm, us |" % title, "|---|---|---|---|"]
    for name, v in win.items():
        base = win[name.replace(" + constraint", "").replace(" (again)", "")]
        lines.append("| %s | %.1f | %.1f - %.1f | %+.1f |" % (name, np.median(v), v.min(), v.max(), np.median(v) - np.median(base)))
    return lines


def host_times():
    from blackbox_mpc_amd import _lib as L
    seq = np.random.default_rng(1).uniform(-1, 1, (N, 1, H, U)).astype(F)
    out = []

    def arms_for(opt):
        arms = {name: _handle(L, user, con, opt=opt) for name, user, con in ARMS}
        arms["built-in reward (again)"] = _handle(L, False, False, opt=opt)      # the off arm's own spread
        return arms
    arms = arms_for(None)
    out += ["### One rollout_particles (bbmpc_evaluate_particles, N %d, no returns), median of 5 windows of 30 calls" % N, ""]
    out += _table("arm", _windows(arms, lambda e, s, t: e.evaluate_particles(s, seq, want_returns=False), 30)) + [""]
    for e, _ in arms.values():
        e.close()
    for opt_name in ("PI2", "CEM"):
        arms = arms_for(getattr(L, "OPT_" + opt_name))
        out += ["### %s control step (%d iterations, N %d), median of 5 windows of 20 steps" % (opt_name, ITERS, N), ""]
        out += _table("arm", _windows(arms, lambda e, s, t: e.optimize(s, t), 20)) + [""]
        for e, _ in arms.values():
            e.close()
    return out


def main():
    if "--kernels" in sys.argv:
        kernels_workload()
        return
    out_dir = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    text = ["# Chance constraint of the particle evaluator (DESIGN.md section 8t): speed", "",
            "Written by tools/chance_constraint_rate.py on an MI355X.  26-200-200-20 model, N %d, P %d, H %d, one agent: %d rows, "
            "trajectory buffer H * S * RS * 4 = %.1f MB per rollout (RS = %d)." % (N, P, H, N * P, H * S * ((N + 63) // 64 * 64) * P * 4 / 1e6,
                                                                                  (N + 63) // 64 * 64 * P), "",
            "## Kernel times (rocprofv3 --kernel-trace, a run of its own)", ""]
    text += kernel_times(out_dir)
    text += ["", "## Host-side times, alternating windows in one process", ""]
    text += host_times()
    path = os.path.join(out_dir, "chance_constraint.md")
    with open(path, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
