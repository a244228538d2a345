"""CPU: the R1CS check's row predicate (zelana_amd/csrc/r1cs_row.h, compiled on
the host by tests/host/r1cs_row_check.cpp) against 256-bit integer arithmetic:
every pairing of the representatives {x, x + r} of a, b and c (k_matvec's
outputs are only reduced below 2r), the values 0, 1 and r - 1, and 1,000
seeded random triples, satisfied and off by one either way.  Built plain and,
where the local g++ links the sanitizer runtimes, with
-fsanitize=address,undefined.  And the product layer's defaults: a BatchProof
is "not checked" and a Groth16Prover does not check unless asked."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "r1cs_row_check.cpp")
# 9 edge pairs + 60 edge/random + 1,000 random triples, each 3 values of c x 8
# representative pairings, + 8 for the high-limb case
CHECKS = (9 + 60 + 1000) * 3 * 8 + 8


def _build(exe, extra):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + extra + ["-o", str(exe), SRC],
                          capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_row_predicate_against_integers(tmp_path):
    exe = tmp_path / "r1cs_row_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == f"ok {CHECKS}", p.stdout + p.stderr
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "r1cs_row_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == f"ok {CHECKS}", p.stdout + p.stderr


def test_product_layer_defaults():
    import inspect

    from zelana_amd.batch_worker import ZBatchProver
    from zelana_amd.prover import BatchProof, BatchPublicInputs, Groth16Prover
    bp = BatchProof(BatchPublicInputs(), bytes(256), 0)
    assert bp.constraints_ok is None and bp.first_unsatisfied is None
    # (no GPU here: the constructor only stores what it is given)
    p = Groth16Prover(None, None, b"vk", circuit=lambda *_: None)
    assert p.check is False
    assert Groth16Prover(None, None, b"vk", circuit=lambda *_: None, check=True).check is True
    assert inspect.signature(ZBatchProver.__init__).parameters["check"].default is False


def test_status_binding_layout():
    """zkmi_r1cs_status crosses the ABI as 14 u64 (first_row, n_bad, a, b, c)."""
    import ctypes

    from zelana_amd import gpu
    from zelana_amd._lib import ROW_NONE, R1CSStatusStruct
    assert ctypes.sizeof(R1CSStatusStruct) == 14 * 8 and ROW_NONE == 2**64 - 1
    arr = (R1CSStatusStruct * 2)()
    arr[0].first_row = ROW_NONE
    arr[1].first_row, arr[1].n_bad = 7, 3
    arr[1].a[0], arr[1].b[3], arr[1].c[1] = 5, 1, 2
    st = gpu._statuses(arr, 2)
    assert st[0] == gpu.R1CSStatus(None, 0, 0, 0, 0) and st[0].ok
    assert st[1] == gpu.R1CSStatus(7, 3, 5, 1 << 192, 2 << 64) and not st[1].ok
