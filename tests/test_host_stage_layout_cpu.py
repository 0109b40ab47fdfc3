"""The layout of a host call's staging buffer (csrc/host_stage_layout.hpp: slot offsets, packing, the optional float4 alignment of a
slot, the total) is plain C++ shared by the C ABI's wrappers (csrc/abi_util.hpp HostStage) and a CPU program:
tests/host_stage_layout_check.cpp (own main) builds a few hundred random slot lists from that header, NULL and
zero-count slots among them, and checks order, alignment, disjointness, the total and the null slots.  Compiled and run
here twice: plainly, and with -fsanitize=address,undefined, where the program's writes into every slot of a real
allocation of `total` floats are checked as well.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

from tests.test_topk_digits_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_host_stage_layout(tmp_path, flags):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = os.path.join(str(tmp_path), "host_stage_layout_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "host_stage_layout_check.cpp"), "-o", exe],
                   check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "all checks held" in res.stdout
