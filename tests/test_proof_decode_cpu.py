"""CPU: the device header's proof decoder (zelana_amd/csrc/proof_decode.h: the
flag, sign and range logic and the Fq / Fq2 square roots that k_proof_decode
runs) compiled for the host and held against verify.cpp's decoder
(tests/host/proof_decode_check.cpp), the way test_pairing_dev_cpu.py holds
pairing.h.  Cases: both signs and infinity for G1 and G2 and every malformed
class of DESIGN.md section 2.9, each with the verdict the rule gives in plain
Python (proof_codec.is_malformed); then the program's own seeded loop of
random byte strings per format.  Built plain and, where the local g++ links
the sanitizer runtimes, with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import proof_codec as PC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zelana_amd", "csrc")
SRCS = [os.path.join(HERE, "host", "proof_decode_check.cpp"), os.path.join(CSRC, "verify.cpp"),
        os.path.join(CSRC, "msm_host.cpp")]
Q = PC.Q


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-mbmi2", "-madx"] + extra + ["-o", str(exe)] + SRCS,
                          capture_output=True, text=True)


def cases():
    """[(fmt, raw)]; the expected verdict of each is proof_codec.is_malformed's"""
    a, b, c = PC.sample_proofs(4100, 1)[0]
    za, zb = np.zeros(8, np.uint64), np.zeros(16, np.uint64)
    out = []
    # well-formed: both signs of every point, every point at infinity, in every format
    for pts in ((a, b, c), (PC.neg_g1(a), b, c), (a, PC.neg_g2(b), c), (a, b, PC.neg_g1(c)), (za, b, c), (a, zb, c),
                (a, b, za), (za, zb, za)):
        for fmt in PC.FORMATS:
            out.append((fmt, PC.encode(fmt, *pts)))
    good = PC.encode(PC.COMPRESSED, a, b, c)
    out += [(PC.COMPRESSED, raw) for raw in PC.malformed_compressed(good).values()]
    # every SWFlags combination on a point and on an all-zero point
    for off, p0 in ((31, 0), (95, 32), (127, 96)):
        for flags in (0x00, 0x40, 0x80, 0xC0):
            out.append((PC.COMPRESSED, PC.patch(good, off, bytes([good[off] & 0x3F | flags]))))
            out.append((PC.COMPRESSED, PC.patch(PC.patch(good, p0, bytes(off - p0)), off, bytes([flags]))))
    unc = PC.encode(PC.UNCOMPRESSED, a, b, c)
    for off, p0 in ((63, 0), (191, 64), (255, 192)):
        for flags in (0x00, 0x40, 0x80, 0xC0):
            out.append((PC.UNCOMPRESSED, PC.patch(unc, off, bytes([unc[off] & 0x3F | flags]))))
            out.append((PC.UNCOMPRESSED, PC.patch(PC.patch(unc, p0, bytes(off - p0)), off, bytes([flags]))))
        stray = PC.patch(PC.patch(unc, p0, bytes(off - p0)), off, b"\x40")
        out.append((PC.UNCOMPRESSED, PC.patch(stray, p0 + 40, b"\x02")))
    # a coordinate >= q in each of the eight positions of each fixed-width format (y of A and C, the four of B, ...)
    for fmt in (PC.UNCOMPRESSED, PC.SOLANA_LE, PC.ALT_BN128_BE):
        raw = PC.encode(fmt, a, b, c)
        order = "big" if fmt == PC.ALT_BN128_BE else "little"
        for k in range(8):
            for v in (Q, Q + 1, 2**254 - 1):
                out.append((fmt, PC.patch(raw, 32 * k, v.to_bytes(32, order))))
            out.append((fmt, PC.patch(raw, 32 * k, (Q - 1).to_bytes(32, order))))  # the largest value allowed
    return out


def test_case_classes_are_not_vacuous():
    cs = cases()
    verdicts = [PC.is_malformed(f, r) for f, r in cs]
    for fmt in PC.FORMATS:
        got = [v for (f, _), v in zip(cs, verdicts) if f == fmt]
        assert got.count(False) >= 8 and got.count(True) >= 8, (fmt, got.count(False), got.count(True))
    a, b, c = PC.sample_proofs(4100, 1)[0]
    bad = PC.malformed_compressed(PC.encode(PC.COMPRESSED, a, b, c))
    assert len(bad) >= 27 and all(PC.is_malformed(PC.COMPRESSED, r) for r in bad.values())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_decode_header_matches_host_decoder(tmp_path):
    cs = cases()
    with open(tmp_path / "cases.txt", "w") as f:
        f.write(f"{len(cs)}\n")
        for fmt, raw in cs:
            f.write(f"{fmt} {int(PC.is_malformed(fmt, raw))} {raw.hex()}\n")
    exe = tmp_path / "proof_decode_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith(f"ok {len(cs)} 8192 "), p.stdout + p.stderr
    accepted = [int(v) for v in p.stdout.split()[3:7]]
    # The shaped strings must reach the accepting paths in every format.  A shaped 32-byte field is < q with
    # probability 7/8 * 0.756 + 1/8 * 0.189 = 0.685, so 0.685^8 = 4.8% of the 4096 fixed-width strings decode (about
    # 200) and 0.685^4 / 2^3 = 2.8% of the compressed ones, whose three x also need a root (about 110, plus the
    # drawn infinities); the loop is seeded, and 32 is far below either figure.
    assert all(n >= 32 for n in accepted), accepted
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "proof_decode_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith(f"ok {len(cs)} 8192 "), p.stdout + p.stderr
