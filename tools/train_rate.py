"""Adam steps/s and whole-`fit` wall time of HipDenseTrainer (hand-written kernels) against DenseTrainer (torch, HIP-graph
replay on: its shipped form) on the same GPU -> profiles/train_hip.md.

Method: both trainers are built once per shape on the same rows; a warm-up fit each (allocations, graph capture paths,
kernel load), then `--rounds` rounds that ALTERNATE the two trainers (torch, hip, torch, hip, ...) in one process, each
round one `fit` of `--epochs` epochs timed by the wall clock around the call (host synchronisation included: the call
returns losses).  Reported per shape: median steps/s, the min .. max spread over the rounds, the median wall time of a
fit, and the ratio of the medians.  The ensemble row fits five members one after the other with either backend, as
SystemDynamicsHandler._train_ensemble does with the torch backend (and did with the hip one).

The ENSEMBLE rows then put that sequential form (one HipDenseTrainer per member: the code of the row above, unchanged) next
to HipEnsembleTrainer -- every member in one launch sequence, the rows uploaded once, each member on its own bootstrap rows
as an index map -- in the same alternating rounds; rates there are MEMBER-steps/s (members x steps of a member).

    python tools/train_rate.py [--rounds 7] [--epochs 2] [--rows 32768] [--out profiles/train_hip_rates.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer, HipEnsembleTrainer      # noqa: E402
from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer       # noqa: E402

SHAPES = [("26-200-200-20 b128", [26, 200, 200, 20], 128, 1),
          ("26-200-200-20 b32", [26, 200, 200, 20], 32, 1),
          ("26-500-500-500-20 b128", [26, 500, 500, 500, 20], 128, 1),
          ("46-200-200-1 b128 (reward net)", [46, 200, 200, 1], 128, 1),
          ("26-200-200-20 b128, 5-member ensemble", [26, 200, 200, 20], 128, 5)]
# (name, dims, batch, members): sequential HipDenseTrainer fits against one HipEnsembleTrainer fit
ENSEMBLE = [("26-200-200-20 b128 E=%d" % E, [26, 200, 200, 20], 128, E) for E in (2, 5, 8)] + \
           [("26-200-200-20 b32 E=%d" % E, [26, 200, 200, 20], 32, E) for E in (2, 5, 8)] + \
           [("26-500-500-500-20 b128 E=5", [26, 500, 500, 500, 20], 128, 5)]


def _params(dims, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.uniform(-1, 1, (i, o)).astype(np.float32) * np.float32(np.sqrt(6.0 / (i + o))) for i, o in zip(dims[:-1], dims[1:])]
    return ws, [np.zeros((o,), np.float32) for o in dims[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    results = []
    for name, dims, B, members in SHAPES:
        acts = [1] * (len(dims) - 2) + [0]
        din = rng.normal(size=(args.rows, dims[0])).astype(np.float32)
        dout = rng.normal(size=(args.rows, dims[-1])).astype(np.float32)
        vin, vout = din[:1024], dout[:1024]
        steps = members * args.epochs * (args.rows // B)

        def fit(backend, seed):
            t0 = time.perf_counter()
            for e in range(members):
                ws, bs = _params(dims, e)
                tr = DenseTrainer(ws, bs, acts, "cuda") if backend == "torch" else HipDenseTrainer(ws, bs, acts)
                tl, _ = tr.fit(din, dout, vin, vout, args.epochs, B, generator_seed=seed)
                assert np.all(np.isfinite(tl))
            return time.perf_counter() - t0

        for backend in ("torch", "hip"):
            fit(backend, 0)
        wall = {"torch": [], "hip": []}
        for r in range(args.rounds):
            for backend in ("torch", "hip"):
                wall[backend].append(fit(backend, 1 + r))
        row = {"shape": name, "steps_per_fit": steps}
        for backend in ("torch", "hip"):
            w = np.asarray(wall[backend])
            row[backend] = {"steps_per_s_median": steps / float(np.median(w)), "steps_per_s_min": steps / float(w.max()),
                            "steps_per_s_max": steps / float(w.min()), "fit_wall_s_median": float(np.median(w))}
        row["hip_over_torch"] = row["hip"]["steps_per_s_median"] / row["torch"]["steps_per_s_median"]
        results.append(row)
        print("%-40s torch %7.0f steps/s (%7.0f .. %7.0f), fit %.3f s | hip %7.0f steps/s (%7.0f .. %7.0f), fit %.3f s | x%.2f"
              % (name, row["torch"]["steps_per_s_median"], row["torch"]["steps_per_s_min"], row["torch"]["steps_per_s_max"],
                 row["torch"]["fit_wall_s_median"], row["hip"]["steps_per_s_median"], row["hip"]["steps_per_s_min"],
                 row["hip"]["steps_per_s_max"], row["hip"]["fit_wall_s_median"], row["hip_over_torch"]), flush=True)
    ensemble = []
    for name, dims, B, members in ENSEMBLE:
        acts = [1] * (len(dims) - 2) + [0]
        din = rng.normal(size=(args.rows, dims[0])).astype(np.float32)
        dout = rng.normal(size=(args.rows, dims[-1])).astype(np.float32)
        vin, vout = din[:1024], dout[:1024]
        rows = [rng.integers(0, args.rows, size=args.rows) for _ in range(members)]
        steps = members * args.epochs * (args.rows // B)

        def fit(path, seed):
            t0 = time.perf_counter()
            if path == "sequential":
                for e in range(members):
                    ws, bs = _params(dims, e)
                    tl, _ = HipDenseTrainer(ws, bs, acts).fit(din, dout, vin, vout, args.epochs, B, generator_seed=seed)
                    assert np.all(np.isfinite(tl))
            else:
                start = [_params(dims, e) for e in range(members)]
                tr = HipEnsembleTrainer([s[0] for s in start], [s[1] for s in start], acts)
                tl, _ = tr.fit(din, dout, vin, vout, args.epochs, B, member_rows=rows, generator_seed=seed)
                assert np.all(np.isfinite(tl))
            return time.perf_counter() - t0

        paths = ("sequential", "one_launch")
        for path in paths:
            fit(path, 0)
        wall = {path: [] for path in paths}
        for r in range(args.rounds):
            for path in paths:
                wall[path].append(fit(path, 1 + r))
        row = {"shape": name, "members": members, "member_steps_per_fit": steps}
        for path in paths:
            w = np.asarray(wall[path])
            row[path] = {"steps_per_s_median": steps / float(np.median(w)), "steps_per_s_min": steps / float(w.max()),
                         "steps_per_s_max": steps / float(w.min()), "fit_wall_s_median": float(np.median(w)),
                         "fit_wall_s_min": float(w.min()), "fit_wall_s_max": float(w.max())}
        row["one_launch_over_sequential"] = row["one_launch"]["steps_per_s_median"] / row["sequential"]["steps_per_s_median"]
        ensemble.append(row)
        print("%-30s sequential %7.0f member-steps/s (%7.0f .. %7.0f), fit %.4f s | one launch %7.0f member-steps/s (%7.0f .. %7.0f), "
              "fit %.4f s | x%.2f"
              % (name, row["sequential"]["steps_per_s_median"], row["sequential"]["steps_per_s_min"], row["sequential"]["steps_per_s_max"],
                 row["sequential"]["fit_wall_s_median"], row["one_launch"]["steps_per_s_median"], row["one_launch"]["steps_per_s_min"],
                 row["one_launch"]["steps_per_s_max"], row["one_launch"]["fit_wall_s_median"], row["one_launch_over_sequential"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rounds": args.rounds, "epochs": args.epochs, "rows": args.rows, "results": results, "ensemble": ensemble}, f, indent=1)


if __name__ == "__main__":
    main()
