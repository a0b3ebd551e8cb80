"""jdsp::DevBuf's failure paths, run for real: without a device every hipMalloc fails, so tests/devbuf_failure.hip
walks them with nothing injected.  It is a stand-alone program whose host side is built under AddressSanitizer and
UndefinedBehaviorSanitizer; a touch of freed memory or a double free on those paths ends it with a report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_devbuf_failure_paths_under_asan_ubsan(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: no allocation fails")
    exe = str(tmp_path / "devbuf_failure")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "devbuf_failure.hip"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "DevBuf failure paths: ok" in run.stdout
