"""CPU: the device header of the nullifier set (zelana_amd/csrc/nullifier_set.h:
the slot function, the store's probes, the scratch grouping and the rules of a
round that nullifier_set.hip's kernels run) compiled for the host, alone, in
tests/host/nullifier_set_check.cpp, driven serially and held against the
sequential model over a Python set (nullifier_set_model).  This pins the
ordered-spend rule before any GPU is involved.  Built plain and, where the
local g++ links the sanitizer runtimes, as the same stand-alone program with
-fsanitize=address,undefined."""
import os
import random
import shutil
import subprocess

import pytest

import nullifier_set_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "nullifier_set_check.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall"] + extra + ["-o", str(exe), SRC],
                          capture_output=True, text=True)


def _spend_line(keys, per_tx, eligible=None):
    ntx = len(keys) // per_tx
    tok = [f"S {per_tx} {ntx}"]
    for t in range(ntx):
        tok.append("0" if eligible is not None and not eligible[t] else "1")
        tok += [k.hex() for k in keys[t * per_tx:(t + 1) * per_tx]]
    return " ".join(tok)


class Script:
    """builds the script and, beside it, what the model expects of every output line"""

    def __init__(self):
        self.lines, self.want = [], []
        self.stored, self.order, self.capacity = set(), [], 0

    def new(self, capacity):
        self.stored, self.order, self.capacity = set(), [], capacity
        self.lines.append(f"N {capacity}")
        self.want.append(["n", str(M.slots_for(capacity))])

    def spend(self, keys, per_tx, eligible=None, check_rounds=True):
        before = set(self.stored)
        res = M.spend_or_refuse(self.stored, self.order, self.capacity, keys, per_tx, eligible)
        self.lines.append(_spend_line(keys, per_tx, eligible))
        if res is None:
            self.want.append(["full", str(len(self.order))])
            return None
        for t, (v, d) in enumerate(zip(*res)):
            self.want.append(["v", str(t), str(v), str(d)])
        accepted, n = M.rounds(before, keys, per_tx, eligible)
        assert accepted == [v == M.ACCEPTED for v in res[0]], "the parallel form disagrees with the model"
        self.want.append(["s", str(n) if check_rounds else None, str(len(self.order))])
        return res

    def contains(self, keys):
        for k in keys:
            self.lines.append(f"C {k.hex()}")
            self.want.append(["c", "1" if k in self.stored else "0"])

    def log(self):
        self.lines.append("L")
        self.want.append(["l", str(len(self.order))] + [k.hex() for k in self.order])

    def text(self):
        return "\n".join(self.lines) + "\n"


def _compare(stdout, want):
    out = [ln.split() for ln in stdout.split("\n") if ln]
    assert out[-1] == ["ok"] and len(out) == len(want) + 1, (len(out), len(want), stdout[-300:])
    for i, (got, w) in enumerate(zip(out, want)):
        assert len(got) == len(w) and all(b is None or a == b for a, b in zip(got, w)), (i, got[:6], w[:6])


def _main_script():
    s = Script()
    # the slot function against its restatement, on hash-like keys and on keys that differ in one word only
    probes = [M.key(i) for i in range(40)] + [M.small_key(i) for i in range(12)] + sum(M.halves(), [])
    probes += [bytes(4 * w) + b"\x01" + bytes(31 - 4 * w) for w in range(8)]
    for slots in (2, 32, 1 << 20, 1 << 32):
        for k in probes:
            s.lines.append(f"H {slots} {k.hex()}")
            s.want.append(["h", str(M.slot(k, slots))])
    # random piles over a tiny universe, a few keys pre-stored, ineligible transfers mixed in
    rng = random.Random(5)
    for case in range(240):
        per_tx = 1 + case % 3
        s.new(64)
        pre = [M.small_key(i) for i in rng.sample(range(12), rng.randrange(0, 4))]
        if pre:
            s.spend(pre, 1)
        for call in range(2):
            keys, eligible = M.random_pile(rng.randrange(1 << 30), rng.randrange(1, 12), per_tx)
            s.spend(keys, per_tx, eligible)
        s.contains([M.small_key(i) for i in range(12)])
        s.log()
    # the chain of 64: 64 rounds, verdicts 0, 3, 0, 3, ...
    s.new(256)
    v, d = s.spend(M.chain(64), 2)
    assert v == [M.ACCEPTED, M.SPENT_IN_CALL] * 32 and d == [0 if t % 2 == 0 else t - 1 for t in range(64)]
    assert s.want[-1][1] == "64"
    # the example, then with B ineligible, then the reasons pile
    s.new(64)
    assert s.spend(M.abc(), 2) == ([0, 3, 0], [0, 0, 0])
    assert s.spend(M.abc(b"abc2"), 2, [True, False, True]) == ([0, 1, 0], [0, 0, 0])
    assert s.spend(M.reasons_pile(), 2) == ([0, 0, 3, 0, 3], [0, 0, 1, 0, 3])
    lo, hi = M.halves()
    assert s.spend(lo + hi, 1)[0] == [0] * 6
    s.contains(lo + hi + [lo[0][:16] + hi[0][16:]])
    s.log()
    return s


def test_model_cases_cover_what_they_claim():
    # the parallel form against the sequential model, as it was checked when the rule was written
    rng = random.Random(1)
    seen = set()
    for _ in range(20000):
        per_tx = rng.randrange(1, 4)
        keys, eligible = M.random_pile(rng.randrange(1 << 30), rng.randrange(1, 10), per_tx, universe=6)
        stored = {M.small_key(i) for i in rng.sample(range(6), rng.randrange(0, 3))}
        s, o = set(stored), []
        v, _ = M.spend(s, o, keys, per_tx, eligible)
        accepted, _ = M.rounds(stored, keys, per_tx, eligible)
        assert accepted == [x == M.ACCEPTED for x in v]
        seen |= set(v)
    assert seen == {0, 1, 2, 3, 4}
    assert M.rounds(set(), M.chain(64), 2)[1] == 64
    home = M.keys_with_home(32, 30, 6)
    assert len(set(home)) == 6 and all(M.slot(k, 32) == 30 for k in home)


def test_header_matches_sequential_model(tmp_path):
    s = _main_script()
    (tmp_path / "script.txt").write_text(s.text())
    exe = tmp_path / "nullifier_set_check"
    r = _build(exe, [])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    p = subprocess.run([str(exe), str(tmp_path / "script.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr
    _compare(p.stdout, s.want)
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "nullifier_set_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san), str(tmp_path / "script.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr
    _compare(p.stdout, s.want)


def test_small_table_wraps_shares_a_home_slot_and_refuses_past_capacity(tmp_path):
    exe = tmp_path / "nullifier_set_check"
    assert _build(exe, []).returncode == 0
    s = Script()
    s.new(16)  # 32 slots
    crowd = M.keys_with_home(32, 30, 6)  # 30, 31, then the probe crosses the table's end: 0, 1, 2, 3
    other = [M.key(i, b"fill") for i in range(40)]
    s.spend(crowd[:5] + other[:3], 2)  # 8 keys, five of them with one home slot
    s.contains(crowd + other[:4])
    for i, k in enumerate(crowd):  # a lookup of the i-th of them walks i + 1 slots (the absent sixth: to the first empty one)
        s.lines.append(f"P {k.hex()}")
        s.want.append(["p", None])
    at = len(s.want)
    s.spend(other[3:11], 1)  # fills to exactly 16
    assert len(s.order) == 16
    s.log()
    assert s.spend([crowd[5]], 1) is None  # one more key: refused
    assert s.spend([other[0], other[1], other[20], other[21]], 2) is None  # refused whole: only its last transfer overflows
    s.spend([other[0], other[20]], 2)  # a refused transfer adds nothing, so this fits
    s.log()
    s.contains(crowd + other[:22])
    (tmp_path / "s.txt").write_text(s.text())
    p = subprocess.run([str(exe), str(tmp_path / "s.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr
    _compare(p.stdout, s.want)
    out = [ln.split() for ln in p.stdout.split("\n") if ln]
    walked = [int(x[1]) for x in out[at - 6:at]]
    assert walked[:5] == [1, 2, 3, 4, 5], "five keys of one home slot sit in consecutive slots across the table's end"
    assert walked[5] >= 6


def test_check_program_refuses_bad_scripts(tmp_path):
    exe = tmp_path / "nullifier_set_check"
    assert _build(exe, []).returncode == 0
    k = M.key(0).hex()
    for bad in ("H 3 " + k,                 # slots no power of two
                "H 4 1234",                 # a short key
                "N 0",                      # capacity
                f"S 1 1 1 {k}",             # no set
                f"N 4\nS 0 1 1",            # per_tx
                f"N 4\nS 5 1 1 {k} {k} {k} {k} {k}",
                f"N 4\nS 1 0",              # no transfers
                f"N 4\nS 1 1 2 {k}",        # eligible is 0 or 1
                f"C {k}",                   # no set
                "L",
                "X"):
        (tmp_path / "bad.txt").write_text(bad + "\n")
        p = subprocess.run([str(exe), str(tmp_path / "bad.txt")], capture_output=True, text=True)
        assert p.returncode == 1 and "ok" not in p.stdout, bad[:40]
