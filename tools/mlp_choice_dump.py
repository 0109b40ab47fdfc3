"""Every result of the kernel-choice case table (tests/test_gpu_mlp_kernel_choice.py) in one .npz, to compare two builds of
the library bit for bit: the same instantiation with the same launch shape gives the same bits.

usage: python tools/mlp_choice_dump.py OUT.npz             (needs a GPU)
       python tools/mlp_choice_dump.py --compare A.npz B.npz   (exit status 1 when a case differs)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump(path):
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib as L
    from tests.test_gpu_mlp_kernel_choice import CASES, run_case
    for k in [k for k in os.environ if k.startswith("BBMPC_MLP_")]:
        del os.environ[k]
    out = {}
    for c in CASES:
        got, _, name, inst, _, _, _ = run_case(L, c, os.environ.__setitem__)
        for k in c["env"]:
            del os.environ[k]
        out[c["id"]] = got
        print("%-32s %s" % (c["id"], inst or "(one-step form)"))
    np.savez(path, **out)


def compare(a, b):
    x, y = np.load(a), np.load(b)
    assert sorted(x.files) == sorted(y.files), (x.files, y.files)
    differ = [k for k in x.files if not np.array_equal(x[k], y[k])]
    for k in differ:
        print("%-32s differs: max |a - b| = %.3e" % (k, float(np.max(np.abs(x[k] - y[k])))))
    print("%d of %d cases identical" % (len(x.files) - len(differ), len(x.files)))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
