"""The read-batch slot arithmetic of the SDK lookup (csrc/lookup_sizing.hpp, what hga_lookup_batch_estimate and
hga_lookup_add_reads share) as a stand-alone host program under AddressSanitizer + UBSan:
tests/native/lookup_sizing_check.cpp walks bases x reads and checks the properties listed at its top."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "lookup_sizing_check.cpp")


@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], []],
                         ids=["asan_ubsan", "plain"])
def test_lookup_sizing_properties(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lookup_sizing_check")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("0 failures")
