"""Measurements behind profiles/elite_carry.md: run on an MI355X with the library built,

    python tools/elite_carry.py [OUT_DIR]            # writes OUT_DIR/elite_carry.md (default profiles/)

1. kernel times of k_elite_save / k_elite_inject (rocprofv3 --kernel-trace around a child process running `--kernels`) at
   N=500, H=30, U=1 (pendulum) and N=1000, H=30, U=6 (26-200-200-20 model), keep = shift = 10 of 50 elites;
2. control-step time with carry on against the SAME handle with carry off, both on the per-iteration route (trace on),
   with and without a mixing matrix, in alternating windows;
3. closed-loop pendulum return with noise_beta = 2 at populations 500, 200, 100, 50, with and without carry, same start
   states and seeds for both arms.
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
os.environ.setdefault("BBMPC_FUSED", "0")        # the pendulum's per-iteration kernels: the route carry takes, for the arm without it too
F = np.float32
H = 30
KEEP = SHIFT = 10


def _pendulum(L, N, A=1, iters=5, k=50, seed=0):
    from blackbox_mpc_amd.engine import Engine
    return Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H,
                  population_size=N, max_iterations=iters, num_elite=k, seed=seed)


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
    """what the profiler watches: 50 control steps of 5 iterations with carry on at both shapes"""
    from blackbox_mpc_amd import _lib as L
    from oracle import oracle_np as O
    eng, s = _pendulum(L, 500), O.pendulum_start_states(1)
    eng.set_elite_carry(KEEP, SHIFT)
    for t in range(50):
        eng.optimize(s, t)
    eng, s = _cheetah(L, 1000)
    eng.set_elite_carry(KEEP, SHIFT)
    for t in range(50):
        eng.optimize(s, t)


def kernel_times(out_dir):
    prof = os.path.join(out_dir, "carry_prof")
    shutil.rmtree(prof, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", prof, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--kernels"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    files = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
    if res.returncode != 0 or not files:
        return ["rocprofv3 run failed (exit %d): no kernel times.\n```\n%s\n```" % (res.returncode, (res.stdout + res.stderr)[-1500:])]
    rows = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if "k_elite_" not in name:
            continue
        kind = "k_elite_inject" if "k_elite_inject" in name else ("k_elite_save<true> (shift)" if "true" in name or "Lb1" in name else "k_elite_save<false> (keep)")
        grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r.get("Grid_Size", 0))
        shape = "N=500, H=30, U=1" if grid <= 512 else "N=1000, H=30, U=6"      # 300 against 1800 threads
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
    lines = ["| workload | matrix | carry off, us | carry on, us | difference, us | windows off (min - max) | windows on (min - max) |",
             "|---|---|---|---|---|---|---|"]
    for label in ("pendulum CEM N=500 H=30 U=1, 5 iterations", "26-200-200-20 model CEM N=1000 H=30 U=6, 5 iterations"):
        for corr in (False, True):
            if label.startswith("pendulum"):
                eng, s = _pendulum(L, 500), O.pendulum_start_states(1)
            else:
                eng, s = _cheetah(L, 1000)
            eng.set_trace(True)                              # both arms on the per-iteration route
            if corr:
                eng.set_sampling_correlation(M)
            win = {False: [], True: []}
            for w in range(6):                               # alternating windows on the same handle; window 0 warms both arms up
                for on in (False, True):
                    eng.set_elite_carry(KEEP if on else 0, SHIFT if on else 0)
                    for t in range(10):
                        eng.optimize(s, t)
                    eng.synchronize()
                    t0 = time.perf_counter()
                    for t in range(200):
                        eng.optimize(s, t)                   # host in / host out: every call ends in a device synchronise
                    if w:
                        win[on].append((time.perf_counter() - t0) / 200 * 1e6)
            off, on = np.asarray(win[False]), np.asarray(win[True])
            lines.append("| %s | %s | %.1f | %.1f | %+.1f | %.1f - %.1f | %.1f - %.1f |" % (
                label, "colored_noise_mixing(30, 2.0)" if corr else "none", np.median(off), np.median(on), np.median(on) - np.median(off),
                off.min(), off.max(), on.min(), on.max()))
            eng.close()
    return lines


def closed_loop():
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.utils.colored_noise import colored_noise_mixing
    A, T, seeds = 16, 200, (0, 1, 2, 3, 4)
    th = np.pi - 2.0 * np.pi * np.arange(A) / A                  # 16 start angles around the circle, hanging down first, at rest
    start = np.stack([np.cos(th), np.sin(th), np.zeros(A)], axis=1).astype(F)
    M = colored_noise_mixing(H, 2.0)
    lines = ["| population | elites | keep = shift | mean return, no carry | with carry | paired difference (carry - none) | its standard error | "
             "std over (start, seed) none / carry | spread of the per-seed means none / carry | worst none / carry | upright none / carry |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for N in (500, 200, 100, 50):
        k = max(2, N // 10)
        kc = max(1, int(round(0.3 * k)))
        rets, up = {False: [], True: []}, {False: 0, True: 0}
        for on in (False, True):
            for seed in seeds:
                eng = _pendulum(L, N, A=A, iters=3, k=k, seed=seed)
                eng.set_sampling_correlation(M)
                if on:
                    eng.set_elite_carry(kc, kc)
                s, total = start, np.zeros(A)
                for t in range(T):
                    _, s, r = eng.optimize(s, t)
                    total += r
                rets[on].append(total)
                up[on] += int(np.sum(s[:, 0] > 0.95))
                eng.close()
        r0, r1 = np.stack(rets[False]), np.stack(rets[True])     # [seeds, A]
        d = (r1 - r0).reshape(-1)
        lines.append("| %d | %d | %d | %.1f | %.1f | %+.1f | %.1f | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %d / %d of %d |" % (
            N, k, kc, r0.mean(), r1.mean(), d.mean(), d.std(ddof=1) / np.sqrt(d.size), r0.std(), r1.std(),
            r0.mean(axis=1).std(), r1.mean(axis=1).std(), r0.min(), r1.min(), up[False], up[True], A * len(seeds)))
    return lines


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    doc = ["# CEM elite carry-over: measurements", "",
           "Produced by `python tools/elite_carry.py` on one MI355X (DESIGN.md section 8h).", "",
           "## Save and inject kernels (rocprofv3 kernel trace, 50 control steps of 5 iterations, first fifth dropped)", "",
           "keep = shift = 10 of 50 elites: 300 threads per launch at H * U = 30, 1800 at H * U = 180.", ""]
    doc += kernel_times(out_dir)                                 # first: the profiled child runs before this process opens the GPU
    doc += ["", "## Control step, host in / host out, per-iteration launches with the trace on (`BBMPC_FUSED=0`)", "",
            "One handle per row, carry switched off and on (keep = shift = 10) in alternating windows of 200 calls after 10 warm-up",
            "calls; median of 5 windows per arm, the first pair of windows dropped. Carry off is the route of the parent commit.", ""]
    doc += step_times()
    doc += ["", "## Closed-loop pendulum, CEM with noise_beta = 2, 3 iterations, H=30, 200 control steps, model = environment", "",
            "16 start angles evenly spaced around the circle (at rest) x 5 seeds, the same for both arms; return = sum of the 200",
            "step rewards; elites = population / 10, keep = shift = 0.3 * elites (iCEM's fraction).", ""]
    doc += closed_loop()
    path = os.path.join(out_dir, "elite_carry.md")
    with open(path, "w") as f:
        f.write("\n".join(doc) + "\n")
    print("\n".join(doc))


if __name__ == "__main__":
    if "--kernels" in sys.argv:
        kernels_workload()
    else:
        main()
