"""How far the persistent pendulum kernel's prefetched-draws rollout reads in the noise buffer (csrc/noise_extent.hpp) is
plain C++ shared by the kernel's addressing and the host's allocation: it is compiled into a program of its own
(tests/noise_extent_check.cpp, with main) and run.  No GPU, nothing loaded into Python.
Covered there, for H in {1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 30, 31}, N in {1, 63, 64, 70, 500, 512} (64 and 512: no slack
rows), 1-3 agents, 1-5 iterations, every trajectory of every agent and iteration, in the last control step of a chunk: the
header's extent equals a brute-force walk of the loop's loads (the CEM / PI2 / RandomSearch loop and the SPSA loop), no
model step uses a block outside its own row, nothing reaches the end of the padded allocation, the pad is at most two
float4 and exactly as large as the last row needs."""
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


def test_noise_extent_matches_a_walk_of_the_loop(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / "noise_extent_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "noise_extent_check.cpp"), "-o", exe],
                   check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "all checks held" in res.stdout
