"""Whole-fit wall time of the HIP trainers with weight decay and early stopping off and on ->
profiles/train_hip.md.  tools/train_rate.py's sibling: 26-200-200-20, batch 128, one network (HipDenseTrainer) and a
5-member ensemble (HipEnsembleTrainer), the rows uploaded once (`set_data`), every timed call one `fit_resident`.

Settings, timed in ALTERNATING rounds in one process (a, b, c, a, b, c, ...) after one warm-up fit each:
  a  defaults
  b  decay on (per-layer lambda, "decoupled": both extra operations of the update kernel)
  c  monitoring on with a patience that never triggers, restore_best on: per epoch the monitor launch and, on every
     improvement, the snapshot copy; at the end the restore launch and the report
  d  (ensemble only) monitoring with patience 2 where two of the five members start from NaN weights: they stop after epoch
     1 and their workgroups return at once for the remaining epochs, the other three run all of them
Reported per setting: the median wall time of a fit, min .. max over the rounds, and the ratio of the median to (a)'s.

`--package-root DIR` times another checkout's build of the package with the same harness (setting (a) only unless it has
the options): how the parent commit is measured in the same session.  `--digest` prints a SHA-256 of the parameters a fixed
default fit leaves, to compare two builds bit for bit.

    python tools/train_reg_rate.py [--rounds 9] [--epochs 8] [--rows 32768] [--out FILE.json] [--package-root DIR] [--digest]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

DIMS, BATCH, MEMBERS = [26, 200, 200, 20], 128, 5
DECAY = dict(weight_decay=[1e-4, 2.5e-4, 5e-4], decay_mode="decoupled")


def _params(seed):
    rng = np.random.default_rng(seed)
    ws = [rng.uniform(-1, 1, (i, o)).astype(np.float32) * np.float32(np.sqrt(6.0 / (i + o))) for i, o in zip(DIMS[:-1], DIMS[1:])]
    return ws, [np.zeros((o,), np.float32) for o in DIMS[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--out", default=None)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--digest", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    has_options = hasattr(T.HipDenseTrainer, "set_weight_decay")
    acts = [1] * (len(DIMS) - 2) + [0]
    rng = np.random.default_rng(0)
    din = rng.normal(size=(args.rows, DIMS[0])).astype(np.float32)
    dout = np.tanh(din @ rng.normal(size=(DIMS[0], DIMS[-1])).astype(np.float32) / 5.0) + 0.1 * rng.normal(size=(args.rows, DIMS[-1])).astype(np.float32)
    dout = dout.astype(np.float32)
    vin, vout = din[:1024], dout[:1024]
    never = dict(patience=args.epochs + 1, restore_best=True)

    def single(**kw):
        tr = T.HipDenseTrainer(*_params(0), acts, **kw)
        tr.set_data(din, dout, vin, vout)
        return tr

    def ensemble(broken=(), **kw):
        start = [_params(e) for e in range(MEMBERS)]
        for e in broken:
            start[e] = ([np.full_like(w, np.nan) for w in start[e][0]], start[e][1])
        tr = T.HipEnsembleTrainer([s[0] for s in start], [s[1] for s in start], acts, **kw)
        tr.set_data(din, dout, vin, vout, member_rows=[rng.integers(0, args.rows, size=args.rows) for _ in range(MEMBERS)])
        return tr

    if args.digest:
        tr = single()
        tl, vl = tr.fit_resident(2, BATCH, generator_seed=7)
        h = hashlib.sha256()
        for p in sum(tr.numpy_params(), []):
            h.update(np.ascontiguousarray(p).tobytes())
        h.update(tl.tobytes() + vl.tobytes())
        print("digest of a default fit (2 epochs, seed 7): %s" % h.hexdigest(), flush=True)

    results = []
    for kind, make in (("single", single), ("5-member ensemble", ensemble)):
        trainers = {"a defaults": make()}
        if has_options:
            trainers["b decay"] = make(**DECAY)
            trainers["c monitor, never stops"] = make(**never)
            if make is ensemble:
                trainers["d monitor, members 1 and 3 stop after epoch 1"] = make(broken=(1, 3), patience=2)
        wall = {name: [] for name in trainers}
        for name, tr in trainers.items():                           # warm-up: allocations, kernel load
            tr.fit_resident(args.epochs, BATCH, generator_seed=0)
        for r in range(args.rounds):
            for name, tr in trainers.items():
                t0 = time.perf_counter()
                tr.fit_resident(args.epochs, BATCH, generator_seed=1 + r)
                wall[name].append(time.perf_counter() - t0)
        base = float(np.median(wall["a defaults"]))
        for name, tr in trainers.items():
            w = np.asarray(wall[name])
            row = {"trainer": kind, "setting": name, "fit_wall_s_median": float(np.median(w)), "fit_wall_s_min": float(w.min()),
                   "fit_wall_s_max": float(w.max()), "over_defaults": float(np.median(w)) / base,
                   "epochs_run": np.atleast_1d(getattr(tr, "epochs_run", args.epochs)).tolist()}
            results.append(row)
            print("%-18s %-48s fit %.4f s (%.4f .. %.4f)  x%.3f of defaults  epochs run %s"
                  % (kind, name, row["fit_wall_s_median"], row["fit_wall_s_min"], row["fit_wall_s_max"], row["over_defaults"],
                     row["epochs_run"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rounds": args.rounds, "epochs": args.epochs, "rows": args.rows, "package_root": args.package_root,
                       "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
