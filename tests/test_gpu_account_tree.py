"""The batched MiMC hash and the GPU-resident account tree (account_tree.hip
over mimc_hash.h; gpu.MimcHasher / AccountTreeDevice and
account_state.DeviceAccountState above them) against zbatch.mimc_hash and
zbatch.SparseTree written one leaf at a time (account_tree_model), then the
closed loop accounts -> batches -> ZBatchProver -> verify_results against a
host restatement of the sequencer's build_witness_with_proofs.  The library
chooses between two launch shapes for the level steps, by the number of writes
alone: one workgroup stepping through all levels (K <= 128: the d3 case and the
first two d32 calls) and a launch per level (the third d32 call, d4).  No
mapping is switchable by a debug variable."""
import ctypes

import numpy as np
import pytest

import account_tree_model as M
from zelana_amd import zbatch as Z
from zelana_amd.r1cs import R

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -1, -4
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hasher(ctx):
    from zelana_amd import gpu
    h = gpu.MimcHasher(ctx)
    yield h
    h.close()


def _p(a):
    from zelana_amd._lib import u64p
    return a.ctypes.data_as(u64p)


# ------------------------------------------------------------------ 1. hash_many
@pytest.mark.parametrize("arity", [1, 2, 3, 4])
def test_hash_many_matches_mimc_hash(ctx, hasher, arity):
    from zelana_amd._lib import lib
    for n in (1, 63, 64, 65, 257):
        tuples = M.hash_inputs(arity, n, n)
        assert n < 16 or all(s in [x for t in tuples for x in t] for s in M.SPECIALS)
        ins = M.words([x for t in tuples for x in t]).reshape(n, 4 * arity)
        out = np.full((n + 3, 4), FILL, np.uint64)
        assert lib().zkmi_mimc_hash_many(ctx.h, hasher.h, n, arity, _p(ins), _p(out)) == 0
        assert (out[n:] == FILL).all(), "words beyond the n x 4 outputs were written"
        got = M.ints(out[:n])
        assert all(v < R for v in got), "an output is not canonical"
        assert got == [M.H(*t) for t in tuples], (arity, n)
        # the same tuples one per call
        for i in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
            assert M.ints(hasher.hash_many([tuples[i]]))[0] == got[i], (arity, n, i)
        assert np.array_equal(hasher.hash_many(tuples), out[:n])  # the wrapper's own marshalling


# ------------------------------------------- 2. apply, one leaf at a time; 3. paths
def _apply_raw(ctx, t, call, depth):
    """zkmi_account_tree_apply into pre-filled buffers; the words beyond the outputs must stay"""
    from zelana_amd._lib import lib
    k = len(call)
    pos = np.array([p for p, _ in call], np.uint64)
    lv = M.words([v for _, v in call])
    sib = np.full((k * depth + 2, 4), FILL, np.uint64)
    old, roots = np.full((k + 2, 4), FILL, np.uint64), np.full((k + 2, 4), FILL, np.uint64)
    rc = lib().zkmi_account_tree_apply(ctx.h, t.h, k, _p(pos), _p(lv), _p(sib), _p(old), _p(roots))
    assert (sib[k * depth:] == FILL).all() and (old[k:] == FILL).all() and (roots[k:] == FILL).all()
    return rc, sib[:k * depth].reshape(k, depth, 4), old[:k], roots[:k]


@pytest.mark.parametrize("name", ["d3", "d32_gpu", "d32_switch", "d4"])
def test_apply_matches_one_by_one_tree(ctx, hasher, name):
    """d3: K = 20 in one workgroup; d32_gpu: K = 1, 127 (one workgroup, across
    the wave boundary), 130 (a launch per level, two workgroups) on one tree;
    d32_switch: K = 128 (the last one-workgroup size) then 129 (the first
    launch-per-level one); d4: K = 1100 on 16 positions (a launch per level,
    past the ordering pass's 1024-position LDS tile)"""
    from zelana_amd import gpu
    depth, calls = M.SEQUENCES[name]
    ref = M.run_one_by_one(name)
    t = gpu.AccountTreeDevice(ctx, hasher, depth, 2 * sum(len(c) for c in calls) * (depth + 1))
    try:
        assert M.ints(t.root()) == [Z.SparseTree(depth).zero[depth]] and t.node_count == 0
        for call, res in zip(calls, ref["calls"]):
            rc, sib, old, roots = _apply_raw(ctx, t, call, depth)
            assert rc == 0
            got_sib, got_old, got_roots = [M.ints(s) for s in sib], M.ints(old), M.ints(roots)
            for k, (w_sib, w_old, w_root) in enumerate(res):
                assert got_old[k] == w_old, (name, k, "replaced leaf")
                assert got_sib[k] == w_sib, (name, k, [i for i in range(depth) if got_sib[k][i] != w_sib[i]])
                assert got_roots[k] == w_root, (name, k, "root")
            assert M.ints(t.root()) == [res[-1][2]]
        # 3. paths and leaves against the final tree, positions never written among them
        tree = ref["tree"]
        written = sorted(tree.leaves)
        never = [p for p in (0, 1, 2, 5, (1 << depth) - 1, (1 << depth) - 3, 1 << (depth - 1)) if p not in tree.leaves]
        if depth > 4:  # d3 and d4 write every position; the never-written ones are d32_gpu's
            assert never, "a position that was never written"
        ask = written[:40] + never + written[:3]
        paths, leaves = t.paths(ask), M.ints(t.leaves(ask))
        for i, p in enumerate(ask):
            w_sib, idx = tree.path(p)
            assert M.ints(paths[i]) == w_sib and leaves[i] == tree.leaves.get(p, 0), (name, p)
            assert Z.merkle_root(leaves[i], M.ints(paths[i]), idx) == M.ints(t.root())[0]
        distinct = {(lv, p >> lv) for p in written for lv in range(depth + 1)}
        assert t.node_count == len(distinct), "every written node is stored once"
    finally:
        t.close()


# ------------------------------------------------------------- 4. a full store
def test_full_store_is_refused_and_left_alone(ctx, hasher):
    from zelana_amd import gpu
    depth = 5
    first = [(3, 10), (2, 11), (31, 12), (3, 13)]
    t = gpu.AccountTreeDevice(ctx, hasher, depth, len(first) * (depth + 1))
    try:
        assert _apply_raw(ctx, t, first, depth)[0] == 0
        count, root = t.node_count, t.root().copy()
        ask = list(range(32))
        paths, leaves = t.paths(ask).copy(), t.leaves(ask).copy()
        room = t.max_nodes - count
        assert depth + 1 <= room < 3 * (depth + 1), "the first call's writes share nodes: one more write fits, three do not"
        rc, sib, old, roots = _apply_raw(ctx, t, [(7, 1), (8, 2), (9, 3)], depth)
        assert rc == ENOMEM
        assert (sib == FILL).all() and (old == FILL).all() and (roots == FILL).all(), "a refused call wrote outputs"
        assert t.node_count == count and np.array_equal(t.root(), root)
        assert np.array_equal(t.paths(ask), paths) and np.array_equal(t.leaves(ask), leaves)
        rc, _, _, roots = _apply_raw(ctx, t, [(3, 99)], depth)  # a call that fits still succeeds
        tree = M.OneByOneTree(depth)
        for p, v in first + [(3, 99)]:
            tree.set(p, v)
        assert rc == 0 and M.ints(roots) == [tree.root()] and t.node_count == count
        # two more writes take the store from half to five sixths full: probe chains on the device
        more = [(12, 21), (20, 22)]
        rc, _, _, roots = _apply_raw(ctx, t, more, depth)
        for p, v in more:
            tree.set(p, v)
        assert rc == 0 and M.ints(roots)[-1] == tree.root() and t.node_count == 20
        paths, leaves = t.paths(ask), M.ints(t.leaves(ask))
        for p in ask:
            assert M.ints(paths[p]) == tree.path(p)[0] and leaves[p] == tree.leaves.get(p, 0), p
        assert _apply_raw(ctx, t, [(1, 1)], depth)[0] == ENOMEM and t.node_count == 20
    finally:
        t.close()


def test_store_filled_to_its_last_slot_on_the_device(ctx, hasher):
    """A depth-32 store of exactly 33 slots takes one write and is full: 33
    lanes claim the 33 slots of one table in one launch (wrap-around, probe
    chains up to the table's length, compare-and-swap races for one slot), and
    every lookup of an absent node then walks the whole full table and ends."""
    from zelana_amd import gpu
    depth = 32
    for pos, leaf in ((2**32 - 1, 77), (0x5A5A5A5A, R + 3)):
        t = gpu.AccountTreeDevice(ctx, hasher, depth, depth + 1)
        try:
            rc, sib, old, roots = _apply_raw(ctx, t, [(pos, leaf)], depth)
            tree = M.OneByOneTree(depth)
            empty_path = tree.path(pos)[0]
            tree.set(pos, leaf % R)
            assert rc == 0 and M.ints(sib[0]) == empty_path and M.ints(old) == [0] and M.ints(roots) == [tree.root()]
            assert t.node_count == depth + 1 == t.max_nodes, "the store is full to its last slot"
            ask = [pos, pos ^ 1, pos ^ (1 << 31), 0, 1, 2**31, 12345]
            ask = [p for i, p in enumerate(ask) if p not in ask[:i]]
            paths, leaves = t.paths(ask), M.ints(t.leaves(ask))
            for i, p in enumerate(ask):
                w_sib, idx = tree.path(p)
                assert M.ints(paths[i]) == w_sib and leaves[i] == tree.leaves.get(p, 0), p
                assert Z.merkle_root(leaves[i], w_sib, idx) == tree.root()
            root = t.root().copy()
            assert _apply_raw(ctx, t, [(pos, 5)], depth)[0] == ENOMEM, "even a rewrite of the same leaf is refused"
            assert np.array_equal(t.root(), root) and np.array_equal(t.paths(ask), paths)
        finally:
            t.close()


# ---------------------------------------------------------------- 5. refusals
def test_abi_refusals(ctx, hasher):
    from zelana_amd import gpu
    from zelana_amd._lib import lib
    L = lib()
    h = ctypes.c_void_p()
    for depth, mx in ((0, 8), (33, 8), (3, 0)):
        assert L.zkmi_account_tree_create(ctx.h, hasher.h, depth, mx, ctypes.byref(h)) == EINVAL, (depth, mx)
    one = M.words([1, 2, 3, 4, 5])
    out = np.full((2, 4), FILL, np.uint64)
    for arity in (0, 5):
        assert L.zkmi_mimc_hash_many(ctx.h, hasher.h, 1, arity, _p(one), _p(out)) == EINVAL
    assert L.zkmi_mimc_hash_many(ctx.h, hasher.h, 0, 2, _p(one), _p(out)) == 0 and (out == FILL).all()
    t = gpu.AccountTreeDevice(ctx, hasher, 3, 64)
    try:
        t.apply([1, 6], [5, 6])
        root, count = t.root().copy(), t.node_count
        for call in ([(8, 1)], [(0, 1), (2**40, 2)]):
            rc, sib, old, roots = _apply_raw(ctx, t, call, 3)
            assert rc == EINVAL and (sib == FILL).all() and (old == FILL).all() and (roots == FILL).all()
        buf = np.full((3 * 3, 4), FILL, np.uint64)
        for pos in ([8], [0, 1, 9], [2**63]):
            arr = np.array(pos, np.uint64)
            assert L.zkmi_account_tree_paths(ctx.h, t.h, arr.size, _p(arr), _p(buf)) == EINVAL
            assert L.zkmi_account_tree_leaves(ctx.h, t.h, arr.size, _p(arr), _p(buf)) == EINVAL
            assert (buf == FILL).all(), "a refused call wrote"
        big = (1 << 16) + 1
        pos, lv = np.zeros(big, np.uint64), np.zeros((big, 4), np.uint64)
        assert L.zkmi_account_tree_apply(ctx.h, t.h, big, _p(pos), _p(lv), None, None, None) == EINVAL
        assert L.zkmi_account_tree_apply(ctx.h, t.h, 0, None, None, None, None, None) == 0
        assert L.zkmi_account_tree_paths(ctx.h, t.h, 0, None, None) == 0
        assert L.zkmi_account_tree_leaves(ctx.h, t.h, 0, None, None) == 0
        assert np.array_equal(t.root(), root) and t.node_count == count
    finally:
        t.close()


def test_no_stream_is_opened(ctx):
    from zelana_amd import gpu
    before = ctx.stream_count()
    h = gpu.MimcHasher(ctx)
    t = gpu.AccountTreeDevice(ctx, h, 6, 256)
    t.apply([1, 2, 1], [4, 5, 6])
    t.paths([0, 63])
    h.hash_many([(1, 2)])
    assert ctx.stream_count() == before
    t.close()
    h.close()
    assert ctx.stream_count() == before


# ------------------------------------------------------------- 6. loop closed
def test_loop_closed(ctx, hasher):
    from zelana_amd import batch_worker as BW
    from zelana_amd import gpu
    from zelana_amd.account_state import DeviceAccountState
    shape = dict(max_transfers=2, max_withdrawals=1, max_shielded=1, depth=3)
    ids = [M.account_id(10 + i, p, 3) for i, p in enumerate((0, 1, 4, 6, 7))]  # 0 and 1 are siblings
    accounts = [(a, 1000 + 100 * i, i) for i, a in enumerate(ids)]
    batches = [
        {"batch_id": 7, "transfers": [(ids[0], ids[1], 50, 11), (ids[0], ids[2], 25, 12)],   # one sender twice; siblings
         "withdrawals": [(ids[3], 0xABCDEF, 30, 13)]},
        {"batch_id": 8, "transfers": [(ids[1], ids[0], 5, 14)], "withdrawals": []},           # an empty transfer slot
        {"batch_id": 9, "transfers": [(ids[4], ids[3], 70, 15), (ids[2], ids[4], 1, 16)],
         "withdrawals": [(ids[4], 0x1234, 9, 17)]},
    ]
    want, want_tree = M.witness_oracle(3, accounts, batches, 2, 1)
    s = DeviceAccountState(ctx, depth=3, max_nodes=512, hasher=hasher)
    w = None
    try:
        assert [s.position_of(a) for a in ids] == [0, 1, 4, 6, 7]
        for a in accounts:
            s.insert(*a)
        with pytest.raises(ValueError):
            s.insert(M.account_id(99, 4, 3), 5)  # another id on position 4
        assert s.root() == want[0]["pre_state_root"]
        # more transfers than slots, and an unknown id, are refused before anything changes
        with pytest.raises(ValueError):
            s.batches([batches[1], {"batch_id": 1, "transfers": [(ids[0], ids[1], 1, 1)] * 3}], max_transfers=2,
                      max_withdrawals=1)
        with pytest.raises(KeyError):
            s.batches([{"batch_id": 1, "transfers": [(ids[0], M.account_id(98, 2, 3), 1, 1)]}], max_transfers=2,
                      max_withdrawals=1)
        assert s.root() == want[0]["pre_state_root"] and s.accounts[ids[0]][1:3] == [1000, 0]
        # numpy integers are taken as they come
        batches[1]["transfers"] = [(ids[1], ids[0], np.int64(5), np.uint64(14))]
        got = s.batches(batches, max_transfers=2, max_withdrawals=1)
        assert all(type(t["amount"]) is int for d in got for t in d["transfers"])
        assert got == want, "the dicts equal the oracle's, field for field"
        assert s.root() == want_tree.root() == got[-1]["post_state_root"]
        for d in got:
            _, _, computed = Z.build(d, witness_only=True, **shape)
            assert all(computed[k] == Z._f(d[k]) for k in Z.PUBLIC), "the circuit recomputes the dict's public values"
        w = BW.ZBatchProver(ctx, got[0], check=True, **shape)
        results = [w.generate_batch_proof(d) for d in got]
        vk = gpu.VerifyingKey(ctx, w.pk.vk_bytes())
        assert BW.verify_results(ctx, vk, results) == [True] * 3
        assert [[int(h, 16) for h in r.public_inputs] for r in results] == [BW.public_values(d) for d in got]
        bad = dict(got[2], transfers=[dict(t) for t in got[2]["transfers"]])
        path = list(bad["transfers"][1]["receiver_path"])
        path[1] = (path[1] + 1) % R
        bad["transfers"][1]["receiver_path"] = path
        with pytest.raises(ValueError):
            w.generate_batch_proof(bad)
    finally:
        if w is not None:
            w.close()
        s.close()
