"""CPU: the device header of note decryption (zelana_amd/csrc/note_crypt.h:
fe25519, X25519, the BLAKE3 derive_key compression, ChaCha20, Poly1305, the
AEAD open and the plaintext parse that note_scan.hip's kernels run) compiled
for the host, alone, in tests/host/note_crypt_check.cpp, driven by a script on
stdin and held against Python integers mod p, the golden vectors and the model
(note_crypt_cases).  The per-op fe25519 cases stand at exactly the bounds the
header states.  Built plain and, where the local g++ links the sanitizer
runtimes, as the same stand-alone program with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

import note_crypt_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "note_crypt_check.cpp")
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
    ops = {op for _, op, _, _ in C.all_cases()}
    assert ops == set(range(1, 16))
    assert [C.TIGHT - 1] * 10 in C.TIGHT_OPERANDS and [C.LOOSE - 1] * 10 in C.LOOSE_OPERANDS
    assert C.fe_val(C.LIMB_MAX) == 2**255 - 1
    assert {len(m) for _, m in C.poly_edge_messages()} == {16, 48}
    assert {k[16:] for k, _ in C.poly_edge_messages()} == {bytes(16), b"\xff" * 16}
    # the low-order points of the extra X25519 cases do give the all-zero secret
    low = [c for c in C.x25519_cases() if c[0].startswith("x25519 low order")]
    assert len(low) == 5
    for _, _, w, _ in low:
        assert C.NC.x25519(C.unwords(w[:8]), C.unwords(w[8:])) == bytes(32)


def test_header_matches_integers_vectors_and_model(tmp_path):
    cases = C.all_cases()
    exe = tmp_path / "note_crypt_check"
    r = _build(exe, [])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    C.check_outputs(cases, _run(exe, cases))
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "note_crypt_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    C.check_outputs(cases, _run(san, cases))


def test_check_program_reads_a_file_and_refuses_bad_scripts(tmp_path):
    exe = tmp_path / "note_crypt_check"
    assert _build(exe, []).returncode == 0
    cases = C.kdf_and_chacha_cases()
    (tmp_path / "s.txt").write_text(C.script(cases))
    p = subprocess.run([str(exe), str(tmp_path / "s.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.endswith("ok\n")
    for bad in ("0 00000000", "16 00000000", "x", "3 123", "3 zz000000", "13 " + "00" * 32 + "ffffffff",
                "14 " + "00" * 44 + "00100000"):
        p = subprocess.run([str(exe)], input=bad + "\n", capture_output=True, text=True)
        assert p.returncode == 1 and "ok" not in p.stdout, bad[:40]
