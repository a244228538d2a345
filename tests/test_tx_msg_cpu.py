"""CPU: the message builders of zelana_amd/csrc/tx_msg.h (the readable and the
legacy message of a transfer and of a withdrawal, as ed25519.hip's kernels
write them on the device) compiled for the host, alone, in
tests/host/tx_msg_check.cpp, fed records on stdin and held byte for byte
against zelana_amd/ed25519.py's builders (tx_msg_cases).  Built plain and,
where the local g++ links the sanitizer runtimes, as the same stand-alone
program with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

import tx_msg_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "tx_msg_check.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + extra + ["-o", str(exe), SRC],
                          capture_output=True, text=True)


def _script(cases):
    return "".join(C.record88(c).hex() + "\n" for c in cases)


def _parse(stdout, n):
    lines = stdout.split("\n")
    assert lines[-2:] == ["ok", ""] and len(lines) == n + 3, (len(lines), n)
    assert lines[-3].startswith("bounds ")
    bounds = tuple(int(v) for v in lines[-3].split()[1:])
    return [tuple(bytes.fromhex(h) for h in ln.split(" ")) for ln in lines[:n]], bounds


def _run(exe, cases):
    p = subprocess.run([str(exe)], input=_script(cases), capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr[-2000:]
    return _parse(p.stdout, len(cases))


def _check(cases, got, bounds):
    for case, g in zip(cases, got):
        want = C.expected(case)
        for kind, (a, b) in enumerate(zip(g, want)):
            assert a == b, (case[0], kind, a, b)
    # the longest and the shortest message of each kind are what the header declares
    want = [C.expected(c) for c in cases]
    lens = [[len(w[k]) for w in want] for k in range(4)]
    assert bounds[:6] == (min(lens[0]), max(lens[0]), min(lens[1]), max(lens[1]), max(lens[2]), max(lens[3]))
    assert bounds[:6] == C.BOUNDS and min(lens[2]) == max(lens[2]) and min(lens[3]) == max(lens[3])
    assert bounds[6] % 16 == 0 and bounds[6] >= max(bounds[1], bounds[3])


def test_cases_cover_the_stated_edges():
    cases = C.all_cases()
    assert {0, 9, 10, 99, 100, 10**19 - 1, 10**19, 2**63, 2**64 - 1, 999, 1001, 10**18 + 1} <= set(C.EDGE_INTS)
    for field in (3, 4, 5):
        assert set(C.EDGE_INTS) <= {c[field] for c in cases}
    ids = {c[1] for c in cases} & {c[2] for c in cases}
    assert {bytes(32), b"\xff" * 32, b"\x0f" * 32, b"\xf0" * 32} <= ids
    l1 = [a for _, a in C.l1_addresses()]
    assert {len(a) - len(a.lstrip(b"\0")) for a in l1} >= {0, 1, 3, 31, 32}
    assert len(C.E.base58(C.be32(58**43 - 1))) == 43 and len(C.E.base58(C.be32(58**43))) == 44
    assert C.E.base58(bytes(32)) == "1" * 32 and len(C.E.base58(b"\xff" * 32)) == 44
    assert sum(c[0].startswith("random record") for c in cases) == 24
    # the digit counts of the random records are spread, not all 19 or 20
    assert len({len(str(c[3])) for c in cases if c[0].startswith("random record")}) >= 6


def test_header_matches_the_model_on_every_byte(tmp_path):
    cases = C.all_cases()
    exe = tmp_path / "tx_msg_check"
    r = _build(exe, [])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    _check(cases, *_run(exe, cases))
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "tx_msg_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    _check(cases, *_run(san, cases))


def test_check_program_reads_a_file_and_refuses_bad_records(tmp_path):
    exe = tmp_path / "tx_msg_check"
    assert _build(exe, []).returncode == 0
    cases = C.all_cases()[:5]
    (tmp_path / "r.txt").write_text(_script(cases))
    p = subprocess.run([str(exe), str(tmp_path / "r.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.endswith("ok\n")
    got, _ = _parse(p.stdout, len(cases))
    assert got == [C.expected(c) for c in cases]
    for bad in ("00", "zz" * 88, "00" * 87, "00" * 89, "0" * 175 + "G"):
        p = subprocess.run([str(exe)], input=bad + "\n", capture_output=True, text=True)
        assert p.returncode == 1 and "ok" not in p.stdout, bad[:40]
