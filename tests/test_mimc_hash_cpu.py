"""CPU: the device header of the MiMC hash and the account tree
(zelana_amd/csrc/mimc_hash.h: the permutation, the sponge, the ordering rule of
a batch of ordered leaf writes and the node store's probes that
account_tree.hip's kernels run) compiled for the host, alone, in
tests/host/account_tree_check.cpp, and held against zbatch.mimc_hash and
zbatch.SparseTree written one leaf at a time (account_tree_model).  This pins
the ordered-update rule before any GPU is involved.  Built plain and, where the
local g++ links the sanitizer runtimes, as the same stand-alone program with
-fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

import account_tree_model as M
from zelana_amd import zbatch as Z
from zelana_amd.r1cs import R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "account_tree_check.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

CPU_SEQUENCES = ("d3", "d3_split", "d32_cpu")
ORDER_CASES = [(3, [p for p, _ in M.SEQUENCES["d3"][1][0]]),
               (32, [p for call in M.SEQUENCES["d32_cpu"][1] for p, _ in call]),
               (1, [0, 1, 1, 0, 0])]


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-g", "-std=c++17"] + extra + ["-o", str(exe), SRC], capture_output=True,
                          text=True)


def _order_brute(depth, pos):
    """the predecessor and last-writer rules by their definitions over the nodes themselves"""
    out = []
    for k, p in enumerate(pos):
        pred = []
        for lv in range(-1, depth):
            node = p if lv < 0 else (p >> lv) ^ 1  # the leaf itself, or the level-lv sibling
            js = [j for j in range(k) if (pos[j] >> max(lv, 0)) == node]
            pred.append(js[-1] if js else -1)
        # the ancestors are nested: once a later write shares level lv it shares every level above
        later =[lv for lv in range(depth + 1) if any((q >> lv) == (p >> lv) for q in pos[k + 1:])]
        m = (min(later) - 1) if later else depth
        out.append([m] + pred)
    return out


def _script():
    """(script text, expectations in output order)"""
    lines, want = [], []
    for arity in (1, 2, 3, 4):
        for t in M.hash_inputs(arity, 18, 0):
            lines.append(f"H {arity} " + " ".join(M.fe_hex(x) for x in t))
            want.append(("h", [M.H(*t)]))
    lines.append("E 32")
    want.append(("e", list(Z.SparseTree(32).zero)))
    for depth, pos in ORDER_CASES:
        lines.append(f"O {depth} {len(pos)} " + " ".join(str(p) for p in pos))
        for k, row in enumerate(_order_brute(depth, pos)):
            want.append(("o", k, row))
    for name in CPU_SEQUENCES:
        depth, calls = M.SEQUENCES[name]
        ref = M.run_one_by_one(name)
        lines.append(f"T {depth} {2 * sum(len(c) for c in calls) * (depth + 1)}")
        for call, res in zip(calls, ref["calls"]):
            lines.append(f"A {len(call)} " + " ".join(f"{p} {M.fe_hex(v)}" for p, v in call))
            for k, (sib, old, root) in enumerate(res):
                want.append(("w", k, [old, root] + sib))
            lines.append("R")
            want.append(("r", None, [res[-1][2]]))
        tree = ref["tree"]
        never = [p for p in (0, 1, 5, (1 << depth) - 1, (1 << depth) - 3) if p not in tree.leaves][:2]
        for p in sorted(tree.leaves)[:12] + never:
            lines.append(f"P {p}")
            sib, idx = tree.path(p)
            want.append(("p", p, [tree.leaves.get(p, 0)] + sib))
            assert Z.merkle_root(tree.leaves.get(p, 0), sib, idx) == tree.root()
    return "\n".join(lines) + "\n", want


def _compare(stdout, want):
    out = stdout.split("\n")
    assert out[len(want)] == "ok", stdout[-400:]
    for line, w in zip(out, want):
        tok = line.split()
        assert tok[0] == w[0], (line[:60], w[0])
        if w[0] == "o":
            assert [int(x) for x in tok[1:]] == [w[1]] + w[2], (line, w)
            continue
        if w[0] in ("w", "p"):
            assert int(tok[1]) == w[1], (line[:60], w[1])
        if w[0] in ("w", "p", "r"):
            tok = tok[1:]
        got = [M.hex_fe(x) for x in tok[1:]]
        assert all(v < R for v in got), "an output is not canonical"
        assert got == w[-1], (w[0], w[1] if len(w) > 2 else None,
                              [i for i, (a, b) in enumerate(zip(got, w[-1])) if a != b], len(got), len(w[-1]))


def test_cases_cover_what_they_claim():
    for arity in (1, 2, 3, 4):
        flat = [x for t in M.hash_inputs(arity, 18, 0) for x in t]
        assert all(s in flat for s in M.SPECIALS)
    for name, (depth, calls) in M.SEQUENCES.items():
        got = M.properties(depth, calls)
        single = len(calls) == 1  # one call has no earlier call: d3 shows that case as d3_split, the same writes
        assert all(v for k, v in got.items() if not (single and k == "stored_from_earlier_call")), (name, got)
        assert all(0 <= p < (1 << depth) for call in calls for p, _ in call)
    depth, calls = M.SEQUENCES["d3"]
    assert len(calls[0]) == 20 and {p for p, _ in calls[0]} == set(range(8))
    assert [w for c in M.SEQUENCES["d3_split"][1] for w in c] == calls[0]
    for name in ("d32_cpu", "d32_gpu"):
        calls = M.SEQUENCES[name][1]
        assert len(calls) == 3 and set(M.EDGE32) <= {p for c in calls for p, _ in c}
        assert {p for p, _ in calls[1]} & {p for p, _ in calls[2]}, "the calls share positions"
    assert [len(c) for c in M.SEQUENCES["d32_gpu"][1]] == [1, 127, 130]
    assert len(M.SEQUENCES["d4"][1][0]) == 1100


def test_header_matches_mimc_hash_and_one_by_one_tree(tmp_path):
    script, want = _script()
    (tmp_path / "script.txt").write_text(script)
    exe = tmp_path / "account_tree_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe), str(tmp_path / "script.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr
    _compare(p.stdout, want)
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "account_tree_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san), str(tmp_path / "script.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr
    _compare(p.stdout, want)


def test_store_fills_to_its_last_slot_and_refuses_past_it(tmp_path):
    exe = tmp_path / "account_tree_check"
    assert _build(exe, []).returncode == 0
    # the bare store: 5 slots, 5 keys; every lookup and claim on the full store ends
    keys = [(3 << 32) | 1, 7, (32 << 32), (1 << 32) | 0xFFFFFFFF, 12345]
    absent = [8, (2 << 32) | 7, 0]
    lines = ["S 5"] + [f"K {k}" for k in keys] + [f"K {keys[1]}"] + [f"F {k}" for k in keys + absent] + \
            [f"K {k}" for k in absent]
    # the tree: a store of exactly depth + 1 nodes takes one write and is full
    v = [M.fe_hex(x) for x in (11, 22)]
    lines += ["T 3 4", f"A 1 5 {v[0]}", "R", "P 5", "P 4", "P 0", f"A 1 5 {v[1]}", f"A 1 2 {v[1]}", "R", "P 5", "P 4", "P 0"]
    (tmp_path / "s.txt").write_text("\n".join(lines) + "\n")
    p = subprocess.run([str(exe), str(tmp_path / "s.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr
    out = [ln.split() for ln in p.stdout.split("\n") if ln]
    assert out[-1] == ["ok"]
    claims = out[:5]
    assert sorted(int(c[1]) for c in claims) == [0, 1, 2, 3, 4] and all(c[2] == "1" for c in claims)
    assert out[5] == ["k", claims[1][1], "0"], "a stored key is found again, not claimed anew"
    finds = out[6:14]
    assert [f[1] for f in finds[:5]] == [c[1] for c in claims] and all(f[1] == "-1" for f in finds[5:])
    assert all(c[1:] == ["-2", "0"] for c in out[14:17]), "a full store gives up"
    t = out[17:]
    tree = Z.SparseTree(3)
    tree.set(5, 11)
    want_paths = [[tree.leaves.get(q, 0)] + tree.path(q)[0] for q in (5, 4, 0)]
    assert t[0][0] == "w" and t[1] == ["r", "4", M.fe_hex(tree.root())]
    before = t[2:5]
    assert [[M.hex_fe(x) for x in ln[2:]] for ln in before] == want_paths
    assert t[5] == ["full", "4"] and t[6] == ["full", "4"]
    assert t[7] == t[1] and t[8:11] == before, "a refused apply changed the state"


def test_check_program_refuses_bad_scripts(tmp_path):
    exe = tmp_path / "account_tree_check"
    assert _build(exe, []).returncode == 0
    one = M.fe_hex(1)
    for bad in ("H 5 " + one,                  # arity
                "H 2 " + one + " 12",          # a short field element
                "E 33",                        # depth
                "T 0 8",                       # depth
                "T 3 0",                       # no slots
                f"A 1 0 {one}",                # no tree
                f"T 3 64\nA 1 8 {one}",        # position >= 2^depth
                f"T 3 64\nA 0",                # no writes
                f"T 3 64\nA 65537 0 {one}",    # more than 2^16 writes
                "T 3 64\nP 9",                 # position
                "O 3 2 1 8",                   # position
                "K 5",                         # no store
                "X"):
        (tmp_path / "bad.txt").write_text(bad + "\n")
        p = subprocess.run([str(exe), str(tmp_path / "bad.txt")], capture_output=True, text=True)
        assert p.returncode == 1 and "ok" not in p.stdout, bad[:40]
