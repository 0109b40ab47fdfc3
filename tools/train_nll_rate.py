"""Whole-fit wall time of the Gaussian-NLL trainers -> profiles/train_hip.md.  tools/train_reg_rate.py's
sibling: a 5-member probabilistic 26-200-200-20 ensemble (mean network + log-variance head per member) at batch 128, every
member on its own bootstrap resample, fitted three ways:
  a  torch     one DenseTrainer(..., logvar_head=...) per member, one after the other (what backend="torch" does)
  b  hip, one  one HipGaussianTrainer per member, one after the other, each on its resampled rows
  c  hip, all  one HipGaussianEnsembleTrainer: all members in one launch sequence (what backend="hip_nll" does)
A timed call is one whole fit of all five members as the handler runs it: trainer construction, the upload of the rows, every
launch, the read-back of the losses -- by the wall clock, ending in the host synchronisation the read-back is.  The three run
one warm-up fit each and then ALTERNATE in one process (a, b, c, a, b, c, ...).  Reported per way: the median, min .. max over
the rounds, Adam steps per second (members x batches x epochs over the median) and the ratio of (a)'s median to it.

    python tools/train_nll_rate.py [--rounds 7] [--epochs 4] [--rows 16384] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

DIMS, BATCH, MEMBERS = [26, 200, 200, 20], 128, 5
BOUNDS = (-10.0, 0.5)


def _member(seed):
    rng = np.random.default_rng(seed)
    shapes = list(zip(DIMS[:-1], DIMS[1:]))
    ws = [rng.uniform(-1, 1, s).astype(np.float32) * np.float32(np.sqrt(6.0 / sum(s))) for s in shapes]
    wv = rng.uniform(-1, 1, shapes[-1]).astype(np.float32) * np.float32(np.sqrt(6.0 / sum(shapes[-1])))
    return ws, [np.zeros((o,), np.float32) for o in DIMS[1:]], (wv, np.zeros((DIMS[-1],), np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer
    if not torch.cuda.is_available():
        raise SystemExit("tools/train_nll_rate.py measures on a GPU and none is visible")
    acts = [1] * (len(DIMS) - 2) + [0]
    rng = np.random.default_rng(0)
    n = args.rows
    din = rng.normal(size=(n, DIMS[0])).astype(np.float32)
    dout = (np.tanh(din @ rng.normal(size=(DIMS[0], DIMS[-1])).astype(np.float32) / 5.0)
            + 0.1 * rng.normal(size=(n, DIMS[-1])).astype(np.float32)).astype(np.float32)
    vin, vout = din[:1024], dout[:1024]
    start = [_member(e) for e in range(MEMBERS)]
    rows = [rng.integers(0, n, size=n) for _ in range(MEMBERS)]

    def fit_torch(seed):
        out = []
        for (ws, bs, head), idx in zip(start, rows):
            tr = DenseTrainer(ws, bs, acts, "cuda", logvar_head=head + BOUNDS)
            out.append(tr.fit(din[idx], dout[idx], vin, vout, args.epochs, BATCH, generator_seed=seed)[0][-1])
        return out

    def fit_hip_one(seed):
        out = []
        for (ws, bs, head), idx in zip(start, rows):
            tr = T.HipGaussianTrainer(ws, bs, acts, logvar_head=head + BOUNDS)
            out.append(tr.fit(din[idx], dout[idx], vin, vout, args.epochs, BATCH, generator_seed=seed)[0][-1])
            tr.close()
        return out

    def fit_hip_all(seed):
        tr = T.HipGaussianEnsembleTrainer([s[0] for s in start], [s[1] for s in start], acts, logvar_heads=[s[2] for s in start],
                                          min_logvar=BOUNDS[0], max_logvar=BOUNDS[1])
        tl, _ = tr.fit(din, dout, vin, vout, args.epochs, BATCH, member_rows=rows, generator_seed=seed)
        tr.close()
        return list(tl[:, -1])

    ways = {"a torch, one DenseTrainer per member": fit_torch, "b hip, one HipGaussianTrainer per member": fit_hip_one,
            "c hip, all members in one launch sequence": fit_hip_all}
    wall, last = {name: [] for name in ways}, {}
    for name, fit in ways.items():                                  # warm-up: allocations, kernel load, library heuristics
        fit(0)
    for r in range(args.rounds):
        for name, fit in ways.items():
            t0 = time.perf_counter()
            last[name] = fit(1 + r)
            wall[name].append(time.perf_counter() - t0)
    steps = MEMBERS * (n // BATCH) * args.epochs
    base = float(np.median(wall["a torch, one DenseTrainer per member"]))
    results = []
    for name in ways:
        w = np.asarray(wall[name])
        row = {"way": name, "fit_wall_s_median": float(np.median(w)), "fit_wall_s_min": float(w.min()), "fit_wall_s_max": float(w.max()),
               "adam_steps_per_s": steps / float(np.median(w)), "torch_over_this": base / float(np.median(w)),
               "last_epoch_train_nll": [float(v) for v in last[name]]}
        assert np.all(np.isfinite(row["last_epoch_train_nll"])), row
        results.append(row)
        print("%-44s fit %.4f s (%.4f .. %.4f)  %.0f steps/s  torch / this x%.2f  last-epoch NLL of member 0 %.4f"
              % (name, row["fit_wall_s_median"], row["fit_wall_s_min"], row["fit_wall_s_max"], row["adam_steps_per_s"],
                 row["torch_over_this"], row["last_epoch_train_nll"][0]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rounds": args.rounds, "epochs": args.epochs, "rows": n, "members": MEMBERS, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
