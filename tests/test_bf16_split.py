"""The host side of the split-bf16 operands (minizero_amd/csrc/bf16_split.h: the rounding hi = bf16(v), lo = bf16(v - hi), and the index of a weight in a
layer's A fragments) — a stand-alone C++ program built here with the address and undefined-behaviour sanitizers; needs no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bf16_split_header(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/csrc/bf16_split_check.cpp")
    exe = str(tmp_path / "bf16_split_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "minizero_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "bf16_split_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bf16_split: ok" in r.stdout
