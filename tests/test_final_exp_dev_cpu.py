"""CPU: the device final exponentiation of verify_each (zelana_amd/csrc/
pairing.h final_exp_is_one and f12_frob2, the routine k_final_exp runs per
lane) compiled for the host and held against verify.cpp
(tests/host/final_exp_dev_check.cpp): Frobenius^2 coefficient by coefficient on
random elements; the verdict on f = 1, f = 0, random and even-coefficient
elements, the Miller values of e(aP, bQ) e(-abP, Q) and of the same with a
wrong scalar, of the reference proof's four pairs for x = 49 (true) and x = 50
(false), and of each multiplied by a random element of Fq6.  Built plain and,
where the local g++ links the sanitizer runtimes, with
-fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

from test_pairing_dev_cpu import cases, write_cases

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "host", "final_exp_dev_check.cpp"),
        os.path.join(HERE, "..", "zelana_amd", "csrc", "verify.cpp")]


def _build(exe, extra):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx"] + extra + ["-o", str(exe)] + SRCS,
                          capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_final_exp_header_matches_host(tmp_path):
    cs = cases()
    assert [e for _, e in cs[:4]] == [1, 0, 1, 0]  # e(aP,bQ)e(-abP,Q), wrong scalar, golden x = 49, x = 50
    write_cases(tmp_path / "cases.txt", cs)
    exe = tmp_path / "final_exp_dev_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith(f"ok 32 {len(cs)}"), p.stdout + p.stderr
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "final_exp_dev_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith(f"ok 32 {len(cs)}"), p.stdout + p.stderr
