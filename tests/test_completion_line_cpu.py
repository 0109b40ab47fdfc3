"""The host side of the resident pendulum kernel's completion line (csrc/completion_line.hpp) is plain C++: it is compiled
into a program of its own (tests/completion_line_check.cpp, with main) and run.  No GPU, nothing loaded into Python.
Covered there: a fully tagged line decodes to the exact five floats (-0.0, a NaN payload, a denormal among them), a line
with one stale word is refused whichever word it is, a line tagged with seq - 1 is refused, and so is a line of the call
65536 numbers earlier (same 16-bit tag), on both sides of the tag's wrap."""
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


def test_completion_line_decode_standalone(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / "completion_line_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "completion_line_check.cpp"), "-o", exe],
                   check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "all checks held" in res.stdout
