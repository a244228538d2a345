"""CPU: the batched verifier's device header (zelana_amd/csrc/pairing.h: Fq12
over the 9 x 29-bit Fq, the lane-per-pair Miller loop of k_miller) compiled
for the host and held against verify.cpp (tests/host/pairing_dev_check.cpp):
products, squares and the sparse line product coefficient by coefficient on
random elements; the header's Miller values through verify.cpp's final
exponentiation on e(aP, bQ) e(-abP, Q) = 1, the same with a wrong scalar, the
reference proof's four pairs (x = 49) and a pair with a point at infinity.
Built plain and, where the local g++ links the sanitizer runtimes, with
-fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_ctypes as O
from test_pairing import ref_proof, ref_vk

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "host", "pairing_dev_check.cpp"),
        os.path.join(HERE, "..", "zelana_amd", "csrc", "verify.cpp")]


def _build(exe, extra):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx"] + extra + ["-o", str(exe)] + SRCS,
                          capture_output=True, text=True)


def neg_g1(p):
    q = np.array(p, np.uint64).copy()
    if q.any():
        q[4:] = O.int_to_limbs((O.Q - O.limbs_to_int(q[4:])) % O.Q)
    return q


def g1_mul(p, k):
    return np.array(O.msm_g1(np.asarray(p, np.uint64).reshape(1, 8), O.ints_to_array([k % O.R])), np.uint64).reshape(8)


def g2_mul(q, k):
    out = np.zeros(16, np.uint64)
    O.lib().oracle_g2_mul(O.P(np.ascontiguousarray(q, np.uint64)), O.P(np.array(O.int_to_limbs(k), np.uint64)),
                          O.P(out))
    return out


def golden_pairs(x=49):
    """e(A, B) e(-alpha, beta) e(-vk_x, gamma) e(-C, delta) of the reference proof"""
    vk = ref_vk()
    (a, b, c), _ = ref_proof()
    vk_x = np.array(O.msm_g1(np.stack([vk["ic"][0], vk["ic"][1]]), O.ints_to_array([1, x])), np.uint64).reshape(8)
    return [(a, b), (neg_g1(vk["alpha"]), vk["beta"]), (neg_g1(vk_x), vk["gamma"]), (neg_g1(c), vk["delta"])]


def cases():
    vk = ref_vk()
    g = np.concatenate([O.int_to_limbs(1), O.int_to_limbs(2)]).astype(np.uint64)  # (1, 2) generates G1
    q = vk["beta"]
    a_, b_ = 123456789, 2**200 + 987654321
    ap, bq = g1_mul(g, a_), g2_mul(q, b_)
    out = [([(ap, bq), (neg_g1(g1_mul(g, a_ * b_)), q)], 1),
           ([(ap, bq), (neg_g1(g1_mul(g, a_ * b_ + 1)), q)], 0),
           (golden_pairs(49), 1),
           (golden_pairs(50), 0),
           ([(ap, bq), (neg_g1(g1_mul(g, a_ * b_)), q), (np.zeros(8, np.uint64), q)], 1),
           ([(ap, np.zeros(16, np.uint64))], 1),
           ([(ap, bq), (np.zeros(8, np.uint64), q)], 0)]
    return out


def write_cases(path, cs):
    with open(path, "w") as f:
        f.write(f"{len(cs)}\n")
        for pairs, expect in cs:
            f.write(f"{len(pairs)} {expect}\n")
            for p, q in pairs:
                f.write(" ".join(str(int(v)) for v in list(p) + list(q)) + "\n")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pairing_header_matches_host_pairing(tmp_path):
    cs = cases()
    write_cases(tmp_path / "cases.txt", cs)
    exe = tmp_path / "pairing_dev_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith(f"ok 64 {len(cs)}"), p.stdout + p.stderr
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "pairing_dev_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith(f"ok 64 {len(cs)}"), p.stdout + p.stderr
