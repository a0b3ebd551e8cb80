"""csrc/ragged_layout.h, the one check between a caller's offset arrays and the batch kernels, run on the host alone:
tests/ragged_layout_selftest.cpp holds the loop the header replaced and compares the two over a seeded sweep of
layouts, walks the boundary cases (among them the inputs on which the old loop overflowed) and pins every message.
It is a stand-alone program built by the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer; a read
past an offset array or a signed overflow inside the check ends it with a report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


def test_ragged_layout_against_the_replaced_loop_under_asan_ubsan(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: sanitizer-built programs run where there is none")
    exe = str(tmp_path / "ragged_layout_selftest")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "ragged_layout_selftest.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert run.stdout.rstrip().endswith("ragged layout: ok")
