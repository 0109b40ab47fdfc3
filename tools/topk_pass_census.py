#!/usr/bin/env python3
"""How many radix passes the CEM elite selection needs, old digit rule against new, on the CPU.

Replays the config-2 closed loop (Pendulum true model, CEM, N = 500, H = 30, 5 iterations, k = 50, one agent) through the
float32 oracle (oracle/oracle_np.py) and, for every selection, restates what csrc/topk.hpp does with the rewards: the
key range as a 512-thread workgroup forms it (per 16-lane row the two smallest keys; the bound is the largest of the rows'
second minima), then the first radix pass under

  * the XOR-prefix rule (digits below the highest bit in which kmin and the bound differ), and
  * the offset rule (digits from the top of span = bound - kmin, csrc/topk_digits.hpp),

for 256, 512 and 1024 first-pass bins.  Printed per rule: the share of selections whose first pass already takes the
boundary bucket whole (no second pass), and how many keys too many that bucket held (mean / max).

    python tools/topk_pass_census.py [--steps 320] [--seed 0]

The old rule's share depends on where the loop spends its time: during the swing-up (the first ~40 control steps) the
rewards of a population spread over several binades and a third of the old rule's selections end after one pass; once the
pendulum is held upright the elites sit close together across a binade or mantissa carry and the share drops.  40 steps
give 33 %, 120 steps about 20 %, the default 320 steps (the length of the device's census) 11 % with 8.7 keys too many on
average -- the device counted 12 % and 9.  The offset rule does not care: 84-87 % at every length.

Left out: the two bound variants of the design table (the exact k-th key as the bound, and the largest over the waves
of their 7th smallest key).  The kernels use the row second-minima only; a tighter bound was out of scope.

No GPU, no library: NumPy only.  The device's own counts are in profiles/cem_select_offset_digits.md."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle_np as O  # noqa: E402

F = np.float32


def reward_keys(r):
    """smaller key == larger reward; -0 folded onto +0 (csrc/topk_digits.hpp reward_key)"""
    u = (np.asarray(r, F) + F(0.0)).view(np.uint32).astype(np.uint64)
    asc = np.where(u >> 31, u ^ 0xFFFFFFFF, u ^ 0x80000000)
    return (~asc) & 0xFFFFFFFF


def key_range(keys, k, nthr=512):
    """(kmin, bound) of block_topk_prepass for N <= nthr (one element per lane)"""
    n = len(keys)
    lanes = np.full(nthr, 0xFFFFFFFF, np.uint64)
    lanes[:n] = keys
    rows = np.sort(lanes.reshape(-1, 16), axis=1)
    rows_ok = min(nthr >> 4, ((n - 2) >> 4) + 1) if n >= 2 else 0
    if 2 * rows_ok >= k:
        return int(keys.min()), int(rows[:rows_ok, 1].max())
    return int(keys.min()), int(keys.max())


def first_pass(keys, k, kmin, bound, rule, width):
    """-> (one pass suffices, keys too many in the boundary bucket)"""
    if rule == "xor":
        top = int(kmin ^ bound).bit_length()
        part = keys[(keys >> top) == (kmin >> top)] if top < 32 else keys
        val = part
    else:
        span = bound - kmin
        top = int(span).bit_length()
        val = keys - kmin
        val = val[val <= span]
    if top == 0:
        return True, 0
    w = min(width, top)
    digits = (val >> (top - w)) & ((1 << w) - 1)
    hist = np.bincount(digits.astype(np.int64), minlength=1 << w)
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, k))               # first bin with cum >= k
    wanted = k - (int(cum[b - 1]) if b else 0)
    excess = int(hist[b]) - wanted
    return excess == 0, excess


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=320)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    N, H, iters, k, A = 500, 30, 5, 50, 1
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
    opt = O.CEM(ev, [-2.0], [2.0], horizon=H, max_iterations=iters, population=N, num_elite=k, num_agents=A, alpha=0.1)
    rng = np.random.default_rng(args.seed)
    state = O.pendulum_start_states(A)
    cases = [("XOR prefix", "xor", 8), ("XOR prefix", "xor", 10), ("offset key - kmin", "off", 8), ("offset", "off", 9),
             ("offset", "off", 10)]
    stats = {c: [] for c in cases}
    for _ in range(args.steps):
        noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 1)).astype(F) for _ in range(iters)]}
        _, state, _ = opt.call(state, noise)
        for tr in opt.trace:
            keys = reward_keys(tr["rewards"][:, 0])
            kmin, bound = key_range(keys, k)
            for c in cases:
                stats[c].append(first_pass(keys, k, kmin, bound, c[1], c[2]))
    print("%d control steps x %d iterations = %d selections" % (args.steps, iters, args.steps * iters))
    print("| digit rule | first-pass bins | one pass suffices | keys too many in the boundary bucket (mean / max) |")
    print("|---|---|---|---|")
    for c in cases:
        ok = np.array([s[0] for s in stats[c]])
        ex = np.array([s[1] for s in stats[c]])
        print("| %s | %d | %.0f %% | %.1f / %d |" % (c[0], 1 << c[2], 100.0 * ok.mean(), ex.mean(), ex.max()))


if __name__ == "__main__":
    main()
