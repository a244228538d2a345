"""CPU: the device header of Ed25519 verification (zelana_amd/csrc/ed25519.h:
SHA-512, reduction mod L, Edwards decompression, doubling, addition,
compression, the double-scalar multiplication and the whole verification that
ed25519.hip's kernels run) compiled for the host, alone, in
tests/host/ed25519_check.cpp, driven by a script on stdin and held against
Python integers, hashlib, libcrypto's golden verdicts and the model
(ed25519_cases).  Built plain and, where the local g++ links the sanitizer
runtimes, as the same stand-alone program with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

import ed25519_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "ed25519_check.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + extra + ["-o", str(exe), SRC],
                          capture_output=True, text=True)


def _run(exe, cases):
    p = subprocess.run([str(exe)], input=C.script(cases), capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr[-2000:]
    lines = p.stdout.split("\n")
    assert lines[-2:] == ["ok", ""] and len(lines) == len(cases) + 2, (len(lines), len(cases))
    return [C.words(bytes.fromhex(ln)) for ln in lines[:-2]]


def test_cases_cover_the_stated_edges():
    cases = C.all_cases()
    assert {op for _, op, _, _ in cases} == set(range(1, 11))
    assert C.SHA_LENS == [0, 1, 111, 112, 127, 128, 129, 239, 240, 256]
    assert {0, C.L - 1, C.L, C.L + 1, 2**252, 2**512 - 1} <= set(C.REDUCE_VALUES)
    assert {C.L - 1, C.L, 2**256 - 1} <= set(C.CANONICAL_VALUES)
    # about half of the random y are on no point, and every golden edge key is among the inputs
    rand = [C.E.decompress(b) for n, b in C.decompress_inputs() if n.startswith("random")]
    assert 6 <= sum(p is None for p in rand) <= len(rand) - 6
    names = {n for n, _ in C.decompress_inputs()}
    assert {"y = p - 1", "y = 2^255 - 1", "golden A not on the curve", "golden A = identity encoded as y = p + 1",
            "golden A = identity with the sign bit set on x = 0"} <= names
    # every reason occurs among the golden cases, and libcrypto and the construction agree on each
    triples = C.golden_triples()
    assert {r for *_, r in triples} == {0, 1, 2, 3}
    assert all(ok == (r == 0) for *_, ok, r in triples)


def test_header_matches_integers_vectors_and_model(tmp_path):
    cases = C.all_cases()
    exe = tmp_path / "ed25519_check"
    r = _build(exe, [])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    C.check_outputs(cases, _run(exe, cases))
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "ed25519_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    C.check_outputs(cases, _run(san, cases))


def test_check_program_reads_a_file_and_refuses_bad_scripts(tmp_path):
    exe = tmp_path / "ed25519_check"
    assert _build(exe, []).returncode == 0
    cases = C.sha_cases()
    (tmp_path / "s.txt").write_text(C.script(cases))
    p = subprocess.run([str(exe), str(tmp_path / "s.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.endswith("ok\n")
    not_a_point = C.le32(2).hex()  # y = 2 is on no point
    assert C.E.decompress(C.le32(2)) is None
    for bad in ("0 00000000", "11 00000000", "x", "2 123", "2 zz000000", "1 ffffffff", "9 " + "00" * 96 + "00100000",
                "6 " + not_a_point):
        p = subprocess.run([str(exe)], input=bad + "\n", capture_output=True, text=True)
        assert p.returncode == 1 and "ok" not in p.stdout, bad[:40]
