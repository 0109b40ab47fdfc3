"""The arithmetic of the elite selection's radix select (csrc/topk_digits.hpp: reward key, key range, per-pass widths,
digits, participation test) is plain C++ shared by the kernels and a CPU program: tests/topk_digits_check.cpp (own main)
restates the workgroup's key range and the multi-pass loop serially from that header and is compiled and run here.  No
GPU, nothing loaded into Python.
Covered there, for N = 1 .. 1100 and k in {1, 2, 50, 64, N}: winner set and sorted order against a brute-force stable sort
on random normal rewards, all equal, two values, +-0 mixed, -1e6 mixed with ordinary rewards, +-inf, denormals and a tie
group across the k-th place; 500 rewards evenly spaced over -128 +- 0.5 with k = 50 take exactly one pass (and two or more
under the rule this one replaced, restated in that file only); span == 0 takes none; nothing takes more than
1 + ceil((32 - W1) / 8)."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cand in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cand) or (cand if os.path.isabs(cand) and os.path.exists(cand) else None)
        if path:
            return path
    return None


def compile_check(out_dir):
    """Compiles tests/topk_digits_check.cpp into out_dir and returns the program's path (the GPU test feeds it traced
    rewards through --passes)."""
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = os.path.join(str(out_dir), "topk_digits_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "topk_digits_check.cpp"), "-o", exe],
                   check=True)
    return exe


def test_topk_digits_match_a_stable_sort(tmp_path):
    exe = compile_check(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "all checks held" in res.stdout
