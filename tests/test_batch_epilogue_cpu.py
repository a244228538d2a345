"""CPU: the batched MSM's host epilogue (msm_host.cpp msm_host_batch_combine,
run by zkmi_msm_batch_wait on a group job's bit sums).  A job of nb x W windows
gives each batch the point of its own W windows -- equal to nb single-job
epilogues, infinity for a batch of all-infinity terms, never the Horner pass
over all nb x W windows (tests/host/batch_epilogue_check.cpp).  Built plain
and, where the local g++ links the sanitizer runtimes, with
-fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "host", "batch_epilogue_check.cpp"),
        os.path.join(HERE, "..", "zelana_amd", "csrc", "msm_host.cpp")]


def _build(exe, extra):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx"] + extra + ["-o", str(exe)] + SRCS,
                          capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_batch_epilogue_per_batch(tmp_path):
    exe = tmp_path / "batch_epilogue_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("ok 8")
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "batch_epilogue_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok 8"), p.stdout + p.stderr
