"""CPU: the probe budget of zkmi_groth16_verify_many (verify.cpp
verify_many_combine_budget, zkmi_ctx_set_verify_probes) driven by a stand-alone
program that plays the GPU's part on the host (tests/host/
verify_budget_check.cpp).  Proofs as test_verify_many_cpu's: the reference's
golden proof repeated, and oracle proofs of square_circuit(x) under one key.
nb = 8, four batches (all valid, one bad, all bad, valid / bad / flagged
mixed), budgets 1, 2, 5 and unlimited: decided and undecided proofs partition
the unflagged ones, every decided verdict is zkmi_groth16_verify's, the probe
count stays within the budget, and the unlimited budget reproduces
verify_many_combine (verdicts and counts).  Built plain and, where the local
g++ links the sanitizer runtimes, with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

from test_verify_many_cpu import golden_set, square_set, write_sets

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "host", "verify_budget_check.cpp"),
        os.path.join(HERE, "..", "zelana_amd", "csrc", "verify.cpp")]


def _build(exe, extra):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx"] + extra + ["-o", str(exe)] + SRCS,
                          capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_budgeted_combine(tmp_path):
    sets = [golden_set(), square_set()]
    write_sets(tmp_path / "sets.txt", sets)
    exe = tmp_path / "verify_budget_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe), str(tmp_path / "sets.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok 2 32"), p.stdout + p.stderr
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "verify_budget_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san), str(tmp_path / "sets.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok 2 32"), p.stdout + p.stderr
