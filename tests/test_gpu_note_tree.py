"""The batched Poseidon hash and the GPU-resident note commitment tree
(note_tree.hip over poseidon_hash.h; gpu.PoseidonHasher / NoteTreeDevice and
shielded.DeviceNoteTree / commit_many / honest_many above them) against
shielded.sponge_hash, the reference's MerkleTree restated one leaf at a time
and a level-by-level rebuild (note_tree_model), then the closed loop
commitments -> tree -> paths -> ShieldedProver.prove_many -> verify_many
against NoteTree and ShieldedTransfer.honest.  The Python oracle costs 1.25 ms
a hash; the sizes are chosen with that in mind."""
import ctypes
import os

import numpy as np
import pytest

import note_tree_model as M
from zelana_amd.r1cs import R

pytestmark = pytest.mark.gpu

EINVAL = -1
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


def _hasher(ctx, mapping):
    """the library's own choice between a quad and a lane per hash, or lanes
    everywhere (ZKMI_DEBUG_NOTE_TREE_NO_QUAD=1, read by zkmi_poseidon_create)"""
    from zelana_amd import shielded as S
    if mapping == "lanes":
        os.environ["ZKMI_DEBUG_NOTE_TREE_NO_QUAD"] = "1"
    try:
        return S.shielded_hasher(ctx)
    finally:
        os.environ.pop("ZKMI_DEBUG_NOTE_TREE_NO_QUAD", None)


@pytest.fixture(scope="module", params=["default", "lanes"])
def hasher(ctx, request):
    """every test below runs under both mappings (the Python references are cached)"""
    h = _hasher(ctx, request.param)
    yield h
    h.close()


def _p(a):
    from zelana_amd._lib import u64p
    return a.ctypes.data_as(u64p)


# ------------------------------------------------------------------ 1. hash_many
@pytest.mark.parametrize("arity", [1, 2, 3, 4])
def test_hash_many_matches_sponge_hash(ctx, hasher, arity):
    from zelana_amd._lib import lib
    for n in (1, 63, 64, 65, 257):
        tuples = M.hash_inputs(arity, n, n)
        assert n < 6 or any(x >= R for t in tuples[:6] for x in t), "the over-range inputs are among them"
        ins = M.words([x for t in tuples for x in t]).reshape(n, 4 * arity)
        out = np.full((n + 3, 4), FILL, np.uint64)
        assert lib().zkmi_poseidon_hash_many(ctx.h, hasher.h, n, arity, _p(ins), _p(out)) == 0
        assert (out[n:] == FILL).all(), "words beyond the n x 4 outputs were written"
        got = M.ints(out[:n])
        assert all(v < R for v in got), "an output is not canonical"
        # the specials, both sides of the wave boundary, the ends, and a spread over the rest
        sample = sorted({i for i in list(range(8)) + [62, 63, 64, 65, n - 2, n - 1] + list(range(8, n, 23))
                         if 0 <= i < n})[:24]
        for i in sample:
            assert got[i] == M.H(*tuples[i]), (arity, n, i)
        # batching against the same call one tuple at a time, on indices outside the sample
        rest = [i for i in range(n) if i not in sample]
        for i in rest[::max(1, len(rest) // 8)][:8]:
            assert M.ints(hasher.hash_many([tuples[i]]))[0] == got[i], (arity, n, i)
        assert np.array_equal(hasher.hash_many(tuples), out[:n])  # the wrapper's own marshalling


def test_hash_many_past_the_quad_threshold(ctx):
    """more tuples than the quad mapping takes (16384): the lane-per-hash
    kernel at a size the library itself picks it for, ragged last workgroup"""
    h, n = _hasher(ctx, "default"), 16384 + 65
    try:
        for arity in (2, 3):
            tuples = M.hash_inputs(arity, n, 5)
            got = M.ints(h.hash_many(tuples))
            for i in list(range(6)) + [63, 64, 127, 128, 8191, 16383, 16384, n - 2, n - 1] + list(range(200, n, 1900)):
                assert got[i] == M.H(*tuples[i]), (arity, i)
            few = [0, 5, 64, 129, 16384, n - 1]  # the same tuples as a short (quad) call
            assert M.ints(h.hash_many([tuples[i] for i in few])) == [got[i] for i in few]
    finally:
        h.close()


def test_batched_note_hashes_match_the_scalar_ones(hasher):
    from zelana_amd import shielded as S
    notes = [(100 + i, bytes([i + 1] * 32), bytes([i + 9] * 32)) for i in range(5)]
    keys = [bytes([40 + i] * 32) for i in range(5)] + [bytes([0xFF] * 32)]  # the last one is >= r
    cms = S.commit_many(hasher, notes)
    assert cms == [S.note_commitment(*n) for n in notes]
    assert S.derive_pk_many(hasher, keys) == [S.derive_pk(k) for k in keys]
    pos = [0, 1, 2, (1 << 32) - 2, 7]
    assert S.nullifier_many(hasher, keys[:5], cms, pos) == [S.nullifier(k, c, p) for k, c, p in zip(keys, cms, pos)]
    assert S.commit_many(hasher, []) == []


# --------------------------------------------- 2. the tree, one leaf at a time
def _empty_leaf(which):
    return 0 if which == "zero" else M.H(0)


@pytest.mark.parametrize("which", ["zero", "h0"])
@pytest.mark.parametrize("seq", [0, 1])
def test_tree_matches_one_by_one_model(ctx, hasher, seq, which):
    from zelana_amd import gpu
    depth, cap, appends = M.SEQUENCES[seq]
    leaves = M.leaf_values(sum(appends), 7 * depth)
    ref = M.run_one_by_one(depth, _empty_leaf(which), leaves)
    t = gpu.NoteTreeDevice(ctx, hasher, depth, cap, _empty_leaf(which))
    try:
        assert M.ints(t.root()) == [ref["empty"][depth]] and t.next_position == 0
        at = 0
        for n in appends:
            first, roots = t.append(leaves[at:at + n])
            assert first == at and t.next_position == at + n
            assert M.ints(roots) == ref["roots"][at:at + n], (at, n)
            assert M.ints(t.root()) == [ref["roots"][at + n - 1]]
            at += n
        want = np.array([M.words(p) for p in ref["paths"]])
        assert np.array_equal(t.paths(range(at)), want)
        order = [(5 * i + 3) % at for i in range(2 * at)] + [0, 0, at - 1]  # permuted, with repeats
        assert np.array_equal(t.paths(order), want[order])
        assert M.ints(t.leaves(0, at)) == ref["leaves"]
        assert M.ints(t.leaves(at - 1, 1)) == ref["leaves"][-1:]
    finally:
        t.close()
    if which == "zero":  # NoteTree's own chain is this tree's
        from zelana_amd.shielded import NoteTree
        assert ref["empty"] == NoteTree(depth).empty


def test_reference_empty_leaf_is_the_default(ctx, hasher):
    from zelana_amd import shielded as S
    t = S.DeviceNoteTree(ctx, depth=4, capacity=16, hasher=hasher)
    try:
        assert t.root() == M.empty_chain(M.H(0), 4)[4] and t.is_valid_root(t.root())
    finally:
        t.close()


# ------------------------------------------------------------- 3. wide append
@pytest.fixture(scope="module")
def wide():
    """303 leaves rebuilt level by level in Python (about 650 hashes), after
    the rebuild itself is held against the one-by-one model in test 2's sizes"""
    h0 = M.H(0)
    for depth, cap, appends in M.SEQUENCES:
        leaves = M.leaf_values(sum(appends), 7 * depth)
        one, re = M.run_one_by_one(depth, h0, leaves), M.RebuiltTree(depth, h0, leaves)
        assert re.root == one["root"] and [re.path(i) for i in range(len(leaves))] == one["paths"]
        assert [re.root_after(k) for k in range(len(leaves))] == one["roots"]
    leaves = M.leaf_values(303, 99)
    return leaves, M.RebuiltTree(32, h0, leaves)


def test_wide_append_matches_rebuild(ctx, hasher, wide):
    from zelana_amd import gpu
    leaves, ref = wide
    t = gpu.NoteTreeDevice(ctx, hasher, 32, 1024, M.H(0))
    try:
        assert t.append(leaves[:3], want_roots=False) == (0, None)
        first, roots = t.append(leaves[3:])
        assert first == 3 and t.next_position == 303
        assert M.ints(t.root()) == [ref.root]
        assert np.array_equal(t.paths(range(303)), np.array([M.words(ref.path(i)) for i in range(303)]))
        got = M.ints(roots)
        assert got[-1] == ref.root
        # the first, the last, both sides of the 128- and 256-leaf boundaries, and a spread
        ks = [3, 4, 127, 128, 129, 255, 256, 257, 302, 301, 64, 100, 191, 200, 288, 37]
        for k in ks:
            assert got[k - 3] == ref.root_after(k), k
    finally:
        t.close()


def test_large_append_equals_chunked_appends(ctx):
    """40,000 leaves in one append (level 1 has 20,000 nodes: past the quad
    threshold, as are the 40,000 per-insertion roots) against the same leaves
    in 40 appends of 1,000, whose launches are all of the sizes the tests above
    hold against the Python models."""
    from zelana_amd import gpu
    h = _hasher(ctx, "default")
    n, chunk = 40000, 1000
    rng = np.random.default_rng(11)
    leaves = rng.integers(0, 2**64, size=(n + 7, 4), dtype=np.uint64)  # any 256-bit values
    a, b = gpu.NoteTreeDevice(ctx, h, 32, 1 << 16, M.H(0)), gpu.NoteTreeDevice(ctx, h, 32, 1 << 16, M.H(0))
    try:
        for t in (a, b):
            t.append(leaves[:7])  # an odd start
        _, roots_a = a.append(leaves[7:])
        roots_b = np.concatenate([b.append(leaves[7 + at:7 + at + chunk])[1] for at in range(0, n, chunk)])
        assert np.array_equal(roots_a, roots_b) and np.array_equal(a.root(), b.root())
        assert np.array_equal(a.root(), roots_a[-1])
        assert np.array_equal(a.leaves(0, n + 7), b.leaves(0, n + 7))
        pos = rng.integers(0, n + 7, size=300)
        assert np.array_equal(a.paths(pos), b.paths(pos))
        # and one path folds to the root through the Python hash
        from zelana_amd.shielded import merkle_root
        p = int(pos[0])
        sibs = [row.tobytes() for row in a.paths([p])[0]]
        assert merkle_root(M.ints(a.leaves(p, 1))[0], sibs, [bool((p >> k) & 1) for k in range(32)]) == M.ints(a.root())[0]
    finally:
        a.close()
        b.close()
        h.close()


# ------------------------------------------------------------------ 4. errors
def test_rejections(ctx, hasher):
    from zelana_amd._lib import lib
    from zelana_amd.shielded import shielded_params
    L = lib()
    table = M.words(M.params_table())
    h = ctypes.c_void_p()
    for rf, rp in ((0, 57), (7, 57), (8, 65), (74, 0)):
        assert L.zkmi_poseidon_create(ctx.h, rf, rp, _p(table), ctypes.byref(h)) == EINVAL, (rf, rp)
    one = M.words([1, 2, 3, 4, 5])
    out = np.full((2, 4), FILL, np.uint64)
    for arity in (0, 5):
        assert L.zkmi_poseidon_hash_many(ctx.h, hasher.h, 1, arity, _p(one), _p(out)) == EINVAL
    assert L.zkmi_poseidon_hash_many(ctx.h, hasher.h, 0, 2, _p(one), _p(out)) == 0 and (out == FILL).all()
    zero = M.words([0])
    for depth, cap in ((0, 1), (33, 1), (3, 0), (3, 9), (32, (1 << 32) + 1)):
        assert L.zkmi_note_tree_create(ctx.h, hasher.h, depth, cap, _p(zero), ctypes.byref(h)) == EINVAL, (depth, cap)
    assert shielded_params()["full"] == 8

    from zelana_amd import gpu
    t = gpu.NoteTreeDevice(ctx, hasher, 3, 5, 0)
    try:
        leaves = M.leaf_values(6, 5)
        t.append(leaves[:3])
        root, path = t.root().copy(), t.paths([1]).copy()
        first = ctypes.c_uint64(77)
        roots = np.full((4, 4), FILL, np.uint64)
        assert L.zkmi_note_tree_append(ctx.h, t.h, 3, _p(M.words(leaves[3:])), ctypes.byref(first), _p(roots)) == EINVAL
        assert (roots == FILL).all() and t.next_position == 3
        assert np.array_equal(t.root(), root) and np.array_equal(t.paths([1]), path)
        assert np.array_equal(t.leaves(0, 3), M.words([v % R for v in leaves[:3]]))
        # n = 0 is a no-op that still reports the position
        assert L.zkmi_note_tree_append(ctx.h, t.h, 0, None, ctypes.byref(first), None) == 0 and first.value == 3
        assert t.next_position == 3 and np.array_equal(t.root(), root)
        sib = np.full((3, 3, 4), FILL, np.uint64)
        for pos in ([3], [0, 1, 3], [2**63]):
            arr = np.array(pos, np.uint64)
            assert L.zkmi_note_tree_paths(ctx.h, t.h, arr.size, _p(arr), _p(sib)) == EINVAL
            assert (sib == FILL).all(), "a refused call wrote siblings"
        assert L.zkmi_note_tree_paths(ctx.h, t.h, 0, None, None) == 0
        lv = np.full((4, 4), FILL, np.uint64)
        for a, n in ((3, 1), (1, 3), (0, 4)):
            assert L.zkmi_note_tree_leaves(ctx.h, t.h, a, n, _p(lv)) == EINVAL and (lv == FILL).all()
        # the last two leaves still fit
        assert t.append(leaves[3:5])[0] == 3 and t.next_position == 5
        ref = M.run_one_by_one(3, 0, leaves[:5])
        assert M.ints(t.root()) == [ref["root"]]
    finally:
        t.close()


# ----------------------------------------------------------------- 5. streams
def test_no_stream_is_opened(ctx):
    from zelana_amd import shielded as S
    before = ctx.stream_count()
    t = S.DeviceNoteTree(ctx, depth=5, capacity=20, empty_leaf=0)
    t.append([1, 2, 3])
    t.paths([0, 2])
    t.hasher.hash_many([(1, 2)])
    assert ctx.stream_count() == before
    t.close()
    t.hasher.close()
    assert ctx.stream_count() == before


def test_root_history_holds_every_insertion_root(ctx, hasher):
    from zelana_amd import shielded as S
    t = S.DeviceNoteTree(ctx, depth=8, capacity=256, empty_leaf=0, hasher=hasher)
    try:
        empty_root = t.root()
        _, r1 = t.append(range(1, 61))
        assert all(t.is_valid_root(r) for r in r1) and t.is_valid_root(empty_root)  # 61 roots
        assert t.is_valid_root(S._b32(r1[7])), "roots are accepted as 32-byte strings too"
        _, r2 = t.append(range(61, 111))
        assert t.root() == r2[-1] and len(set(r1 + r2)) == 110
        # RootHistory keeps ROOT_HISTORY_SIZE = 100: the 50 newest and the 50 before them
        assert all(t.is_valid_root(r) for r in r2 + r1[10:])
        assert not any(t.is_valid_root(r) for r in r1[:10] + [empty_root])
        assert t.get(5) == 6 and t.next_position == 110
    finally:
        t.close()


# ------------------------------------------------------------- 6. loop closed
def test_loop_closed_small(ctx, hasher):
    from zelana_amd import shielded as S
    b = lambda v: bytes([v] * 32)  # noqa: E731
    specs = [(100 + 10 * i, b(10 + i), b(20 + i), i) for i in range(4)]
    outs = [[S.OutputNote(150, b(30), b(40)), S.OutputNote(57, b(31), b(41))],
            [S.OutputNote(200, b(32), b(42)), S.OutputNote(7, b(33), b(43))]]
    want_notes = S.NoteTree(3).spend_notes(specs)
    want = [S.ShieldedTransfer.honest(want_notes[0:2], outs[0]), S.ShieldedTransfer.honest(want_notes[2:4], outs[1])]
    tree = S.DeviceNoteTree(ctx, depth=3, capacity=8, empty_leaf=0, hasher=hasher)
    stale_tree = S.DeviceNoteTree(ctx, depth=3, capacity=8, empty_leaf=0, hasher=hasher)
    sp = None
    try:
        notes = tree.spend_notes(specs)
        assert notes == want_notes
        with pytest.raises(ValueError):
            tree.spend_notes([(1, b(1), b(2), 7)])  # not the next free position
        got = S.honest_many(hasher, [notes[0:2], notes[2:4]], outs)
        assert got == want, "the path folded on the device"
        assert S.honest_many(hasher, [notes[0:2], notes[2:4]], outs, tree=tree) == want, "the tree's root"
        assert S.honest_many(hasher, [notes[0:1]], [outs[0][:1]], fees=[9])[0] == \
            S.ShieldedTransfer.honest(want_notes[0:1], outs[0][:1], 9)
        # paths taken after two notes, the root after four: a stale path
        old = stale_tree.spend_notes(specs[:2])
        stale_tree.spend_notes(specs[2:])
        stale = S.honest_many(hasher, [old], [outs[0]], tree=stale_tree)[0]
        assert stale.merkle_root == want[0].merkle_root and stale.inputs[0].merkle_path != notes[0].merkle_path
        assert stale.nullifiers == want[0].nullifiers

        sp = S.ShieldedProver(ctx, (3, 3, 2), seed=3, check=True)
        proofs = sp.prove_many(got + [stale], [11, 12, 13])
        assert [p.constraints_ok for p in proofs] == [True, True, False]
        assert proofs[2].first_unsatisfied == sp.rows["root"][0]
        assert sp.verify_many(proofs) == [True, True, False]
    finally:
        if sp is not None:
            sp.close()
        tree.close()
        stale_tree.close()
