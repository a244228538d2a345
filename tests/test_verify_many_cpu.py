"""CPU: the host half of zkmi_groth16_verify_many (verify.cpp
verify_many_combine: one final exponentiation for a batch, bisection when the
combined check fails) driven by a stand-alone program that plays the GPU's
part with the device header compiled for the host
(tests/host/verify_many_check.cpp).  Proofs: the reference's golden proof
(x = 49) repeated, and oracle proofs of square_circuit(x) for several x under
one key.  Fixed weights.  nb = 5: all valid, every single bad position, two
bad, all bad, a proof flagged by point validation; nb = 8 with one bad proof
costs at most 1 + 2 ceil(log2 nb) final exponentiations; a zero weight is
refused.  Expected verdicts are zkmi_groth16_verify's.  Built plain and, where
the local g++ links the sanitizer runtimes, with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_groth16 import _oracle_prove, _setup
from test_pairing import ref_proof, ref_vk
from test_verify_cpu import compressed_vk
from zelana_amd.r1cs import square_circuit

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "host", "verify_many_check.cpp"),
        os.path.join(HERE, "..", "zelana_amd", "csrc", "verify.cpp")]


def _build(exe, extra):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx"] + extra + ["-o", str(exe)] + SRCS,
                          capture_output=True, text=True)


def square_set(xs=(3, 7, 11), seed=77):
    """(vk bytes, [(inputs, a, b, c)]) of oracle proofs of square_circuit(x) under one key"""
    cs, _ = square_circuit(xs[0])
    opk, _, rng, (st, keep) = _setup(cs, seed)
    buf = np.zeros(4096, np.uint8)
    n = O.lib().oracle_vk_serialize(opk, 1, O.P(buf), 4096)
    proofs = []
    for x in xs:
        _, z = square_circuit(x)
        zz = np.array([O.int_to_limbs(v) for v in z], np.uint64)
        a, b, c = _oracle_prove(opk, st, zz, rng.fr(), rng.fr())
        proofs.append(([x * x % O.R], a, b, c))
    del keep
    return bytes(buf[:n]), proofs


def golden_set():
    (a, b, c), x = ref_proof()
    return compressed_vk(ref_vk()), [([x], a, b, c)]


def write_sets(path, sets):
    with open(path, "w") as f:
        f.write(f"{len(sets)}\n")
        for vkb, proofs in sets:
            f.write(f"{len(vkb)}\n" + " ".join(str(v) for v in vkb) + "\n")
            f.write(f"{len(proofs[0][0])} {len(proofs)}\n")
            for ins, a, b, c in proofs:
                words = [w for v in ins for w in O.int_to_limbs(v)] + list(a) + list(b) + list(c)
                f.write(" ".join(str(int(w)) for w in words) + "\n")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_verify_many_combine_and_bisect(tmp_path):
    sets = [golden_set(), square_set()]
    write_sets(tmp_path / "sets.txt", sets)
    exe = tmp_path / "verify_many_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe), str(tmp_path / "sets.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok 2 28"), p.stdout + p.stderr
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "verify_many_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san), str(tmp_path / "sets.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok 2 28"), p.stdout + p.stderr
