"""The arithmetic the all-wave route of the elite selection adds (csrc/topk_digits.hpp: topk_pick16, the scan's pick in
every wave; topk_whole_bucket_in, the one-pass predicate) is
plain C++ shared by the kernel and a CPU program: tests/topk_wave_list_check.cpp (own main) restates the route serially
from that header and checks it against the selection as it was and against a plain sort -- random populations,
populations that straddle a binade, all-equal rewards, -1e6 entries, and k - 1 / k / k + 1 copies of the boundary value.
The route must be taken exactly when the old selection reports one pass with eq_total == remaining, its list must equal
the old one element for element, and every case it declines must be one the old code handles.
No GPU, nothing loaded into Python."""
import os
import subprocess

from tests.test_topk_digits_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_list_matches_the_old_selection_and_a_sort(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = os.path.join(str(tmp_path), "topk_wave_list_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "topk_wave_list_check.cpp"), "-o", exe],
                   check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "all checks held" in res.stdout
