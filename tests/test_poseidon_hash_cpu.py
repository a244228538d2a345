"""CPU: the device header of the Poseidon hash and the note tree
(zelana_amd/csrc/poseidon_hash.h: the permutation, the sponge, the tree's index
arithmetic, the batch rehash and the per-insertion fold that note_tree.hip's
kernels run) compiled for the host, alone, in tests/host/note_tree_check.cpp,
and held against shielded.sponge_hash and the reference's MerkleTree restated
one leaf at a time (note_tree_model.OneByOneTree).  This pins the
per-insertion rule and the batch rehash before any GPU is involved.  Built
plain and, where the local g++ links the sanitizer runtimes, with
-fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

import note_tree_model as M
from zelana_amd.r1cs import R
from zelana_amd.shielded import NoteTree, _b32, merkle_root, shielded_params

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "note_tree_check.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-g", "-std=c++17"] + extra + ["-o", str(exe), SRC], capture_output=True,
                          text=True)


def _params_cmd():
    p = shielded_params()
    return f"C {p['full']} {p['partial']} " + " ".join(M.fe_hex(c) for c in M.params_table())


def _script():
    """(script text, expectations in output order)"""
    lines, want = [_params_cmd()], []
    for arity in (1, 2, 3, 4):
        for t in M.hash_inputs(arity, 10, 0):
            lines.append(f"H {arity} " + " ".join(M.fe_hex(x) for x in t))
            want.append(("h", [M.H(*t)]))
    # the empty-subtree chains: NoteTree's (empty leaf 0) and the reference's (H(0), merkle.rs:126-153)
    lines.append("E 32 " + M.fe_hex(0))
    want.append(("e", list(NoteTree(32).empty)))
    h0 = M.H(0)
    lines.append("E 32 " + M.fe_hex(h0))
    want.append(("e", M.empty_chain(h0, 32)))
    for depth, cap, appends in M.SEQUENCES:
        leaves = M.leaf_values(sum(appends), 7 * depth)
        ref = M.run_one_by_one(depth, h0, leaves)
        lines.append(f"T {depth} {cap} " + M.fe_hex(h0))
        at = 0
        for n in appends:
            lines.append(f"A {n} " + " ".join(M.fe_hex(v) for v in leaves[at:at + n]))
            want.append(("a", at, ref["roots"][at:at + n] + [ref["roots"][at + n - 1]]))
            at += n
        lines.append("P")
        for pos in range(len(leaves)):
            want.append(("p", pos, [ref["leaves"][pos]] + ref["paths"][pos]))
        # each path folds to the root through the circuit's own fold
        for pos in range(len(leaves)):
            bits = [bool((pos >> level) & 1) for level in range(depth)]
            assert merkle_root(ref["leaves"][pos], [_b32(s) for s in ref["paths"][pos]], bits) == ref["root"]
    return "\n".join(lines) + "\n", want


def _compare(stdout, want):
    out = stdout.split("\n")
    assert out[len(want)] == "ok", stdout[-400:]
    for line, w in zip(out, want):
        tok = line.split()
        assert tok[0] == w[0], (line[:60], w[0])
        if w[0] in ("a", "p"):
            assert int(tok[1]) == w[1], (line[:60], w[1])
            tok = tok[1:]
        got = [M.hex_fe(x) for x in tok[1:]]
        assert all(v < R for v in got), "an output is not canonical"
        assert got == w[-1], (w[0], w[1] if len(w) > 2 else None,
                              [i for i, (a, b) in enumerate(zip(got, w[-1])) if a != b], len(got), len(w[-1]))


def test_cases_cover_what_they_claim():
    for arity in (1, 2, 3, 4):
        flat = [x for t in M.hash_inputs(arity, 10, 0) for x in t]
        assert all(s in flat for s in M.SPECIALS) and any(x >= R for x in flat)
    for depth, cap, appends in M.SEQUENCES:
        leaves = M.leaf_values(sum(appends), 7 * depth)
        assert any(v >= R for v in leaves) and len({v % R for v in leaves}) == len(leaves)
    assert sum(M.SEQUENCES[0][2]) == M.SEQUENCES[0][1], "the small tree is filled to its last leaf"
    # the ranges start at odd positions and cross subtree boundaries of several heights
    starts = [sum(M.SEQUENCES[1][2][:i]) for i in range(len(M.SEQUENCES[1][2]))]
    assert starts == [0, 1, 3, 8] and any(s & 1 for s in starts)


def test_header_matches_sponge_and_one_by_one_tree(tmp_path):
    script, want = _script()
    (tmp_path / "script.txt").write_text(script)
    exe = tmp_path / "note_tree_check"
    r = _build(exe, [])
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe), str(tmp_path / "script.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr
    _compare(p.stdout, want)
    # the same stand-alone program under ASan + UBSan, when this g++ can link them
    san = tmp_path / "note_tree_check_san"
    r = _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        print("sanitizer build not available here; ran the plain build only:", r.stderr[-300:])
        return
    p = subprocess.run([str(san), str(tmp_path / "script.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr
    _compare(p.stdout, want)


def test_check_program_refuses_bad_scripts(tmp_path):
    exe = tmp_path / "note_tree_check"
    assert _build(exe, []).returncode == 0
    for bad in ("H 2 " + M.fe_hex(1) + " " + M.fe_hex(2),            # no parameter set
                _params_cmd() + "\nH 5 " + M.fe_hex(1),                # arity
                _params_cmd() + f"\nT 3 9 {M.fe_hex(0)}",              # capacity above 2^depth
                _params_cmd() + f"\nT 3 2 {M.fe_hex(0)}\nA 3 " + " ".join([M.fe_hex(1)] * 3)):  # past the capacity
        (tmp_path / "bad.txt").write_text(bad + "\n")
        p = subprocess.run([str(exe), str(tmp_path / "bad.txt")], capture_output=True, text=True)
        assert p.returncode == 1 and "ok" not in p.stdout, bad[:40]
