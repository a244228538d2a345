"""The GPU-resident nullifier set (nullifier_set.hip over nullifier_set.h;
gpu.NullifierSetDevice above it) against the sequential model over a Python
set (nullifier_set_model): contains / spend over consecutive calls on one set
at sizes on both sides of the switch between the one-workgroup rounds and a
launch pair per round, chains that need one round per transfer, the reasons of
refusals in key order, a small table filled to its last key with probes that
cross its end, the log's order, and the argument errors.  The raw ABI calls
write into pre-filled buffers; the words beyond the outputs must stay as they
were."""
import ctypes

import numpy as np
import pytest

import nullifier_set_model as M

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -1, -4
FILL32, FILL8 = np.uint32(0xA5A5A5A5), np.uint8(0xA5)
ONE_WG = 128  # nullifier_set.hip NS_ONE_WG: the rounds of more transfers take a launch pair each


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


def _u8(a):
    from zelana_amd._lib import u8p
    return a.ctypes.data_as(u8p)


def _u32(a):
    from zelana_amd._lib import u32p
    return a.ctypes.data_as(u32p)


def _kb(keys):
    return np.frombuffer(b"".join(keys), np.uint8).copy() if keys else np.zeros(32, np.uint8)


class Raw:
    """a set driven through the C ABI, with guard words behind every output"""
    PAD = 5

    def __init__(self, ctx, capacity):
        from zelana_amd._lib import lib, vp
        self.L, self.ctx, self.h = lib(), ctx, vp()
        rc = self.L.zkmi_nullifier_set_create(ctx.h, capacity, ctypes.byref(self.h))
        assert rc == 0, self.L.zkmi_last_error()

    def info(self):
        out = np.zeros(3, np.uint64)
        assert self.L.zkmi_nullifier_set_info(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == 0
        return [int(v) for v in out]

    def contains(self, keys):
        n = len(keys)
        out = np.full(n + self.PAD, FILL8, np.uint8)
        rc = self.L.zkmi_nullifier_set_contains(self.ctx.h, self.h, n, _u8(_kb(keys)), _u8(out))
        assert rc == 0, self.L.zkmi_last_error()
        assert (out[n:] == FILL8).all(), "contains wrote past its output"
        assert set(out[:n].tolist()) <= {0, 1}
        return [bool(v) for v in out[:n]]

    def spend(self, keys, per_tx, eligible=None):
        """-> (rc, verdicts, details, rounds); on a refusal the outputs must be untouched"""
        ntx = len(keys) // per_tx
        v, d = np.full(ntx + self.PAD, FILL32, np.uint32), np.full(ntx + self.PAD, FILL32, np.uint32)
        rounds = np.full(1 + self.PAD, FILL32, np.uint32)
        el = None if eligible is None else np.array([1 if e else 0 for e in eligible], np.uint8)
        rc = self.L.zkmi_nullifier_set_spend(self.ctx.h, self.h, ntx, per_tx, _u8(_kb(keys)),
                                             None if el is None else _u8(el), _u32(v), _u32(d), _u32(rounds))
        assert (v[ntx:] == FILL32).all() and (d[ntx:] == FILL32).all() and (rounds[1:] == FILL32).all(), \
            "spend wrote past its outputs"
        if rc != 0:
            assert (v == FILL32).all() and (d == FILL32).all() and rounds[0] == FILL32, "a refused spend wrote outputs"
            return rc, None, None, None
        return rc, v[:ntx].tolist(), d[:ntx].tolist(), int(rounds[0])

    def log(self, first, n):
        out = np.full((n + 1) * 32, FILL8, np.uint8)
        rc = self.L.zkmi_nullifier_set_log(self.ctx.h, self.h, first, n, _u8(out))
        assert (out[n * 32:] == FILL8).all(), "log wrote past its output"
        return rc, [out[32 * i:32 * i + 32].tobytes() for i in range(n)]

    def close(self):
        self.L.zkmi_nullifier_set_destroy(self.h)


class Both:
    """the raw set beside the model's set and log; every call is checked against the model"""

    def __init__(self, ctx, capacity):
        self.raw, self.capacity = Raw(ctx, capacity), capacity
        self.stored, self.order = set(), []

    def spend(self, keys, per_tx, eligible=None):
        before = set(self.stored)
        want = M.spend_or_refuse(self.stored, self.order, self.capacity, keys, per_tx, eligible)
        rc, v, d, rounds = self.raw.spend(keys, per_tx, eligible)
        if want is None:
            assert rc == ENOMEM
            return None
        assert rc == 0
        bad = [t for t in range(len(v)) if (v[t], d[t]) != (want[0][t], want[1][t])]
        assert not bad, (bad[:5], [(v[t], d[t], want[0][t], want[1][t]) for t in bad[:5]])
        assert rounds == M.rounds(before, keys, per_tx, eligible)[1]
        assert self.raw.info() == [self.capacity, M.slots_for(self.capacity), len(self.order)]
        return v, d, rounds

    def check_state(self, probes):
        assert self.raw.contains(probes) == [k in self.stored for k in probes]
        rc, log = self.raw.log(0, len(self.order))
        assert rc == 0 and log == self.order

    def close(self):
        self.raw.close()


# ------------------------------------------------- 1. against the model, by size
@pytest.mark.parametrize("per_tx", [1, 2, 4])
def test_consecutive_calls_match_model(ctx, per_tx):
    """sizes on both sides of ONE_WG = 128 (and of a 64-lane wave and a 256-lane block), three calls each on one set"""
    b = Both(ctx, 8192)
    try:
        hit_stored = hit_in_call = 0
        for ntx in (1, 63, 64, 65, 129, 300):
            for call in range(3):
                keys, eligible = M.mixed_pile(ntx * 10 + per_tx, ntx, per_tx, call)
                v, _, _ = b.spend(keys, per_tx, eligible)
                hit_stored += v.count(M.SPENT_STORED)
                hit_in_call += v.count(M.SPENT_IN_CALL)
                b.check_state(keys[:64] + [M.key(i, b"absent") for i in range(8)])
        assert hit_stored > 20 and hit_in_call > 20, "later calls must hit keys stored by earlier ones"
        assert len(b.order) > 1000
    finally:
        b.close()


@pytest.mark.parametrize("ntx", [ONE_WG - 1, ONE_WG, ONE_WG + 1])
def test_dense_conflicts_on_both_sides_of_the_switch(ctx, ntx):
    """a tiny key universe: every kind of refusal, several rounds, in both launch shapes"""
    b = Both(ctx, 64)
    try:
        pool = [M.small_key(i) for i in range(40)]
        b.spend(pool[:3], 1)
        seen = set()
        for per_tx in (1, 2, 3):
            keys, eligible = M.random_pile(ntx + per_tx, ntx, per_tx, pool=pool[:10 * per_tx])
            v, _, rounds = b.spend(keys, per_tx, eligible)
            seen |= set(v)
        assert seen == {0, 1, 2, 3, 4}
        b.check_state(pool)
    finally:
        b.close()


# ------------------------------------------------------------------ 2. chains
@pytest.mark.parametrize("n", [64, 200])
def test_chain_takes_a_round_per_transfer(ctx, n):
    """64 runs in the one workgroup, 200 iterates the launch pair; verdicts 0, 3, 0, 3, ..."""
    assert 64 <= ONE_WG < 200
    b = Both(ctx, 512)
    try:
        v, d, rounds = b.spend(M.chain(n), 2)
        assert rounds == n
        assert v == [M.ACCEPTED, M.SPENT_IN_CALL] * (n // 2)
        assert d == [0 if t % 2 == 0 else t - 1 for t in range(n)]
        b.check_state(M.chain(n)[:20])
    finally:
        b.close()


def test_example_and_ineligible_middle(ctx):
    b = Both(ctx, 64)
    try:
        assert b.spend(M.abc(), 2) == ([0, 3, 0], [0, 0, 0], 3)  # A spends, B is refused, so C spends
        # with B ineligible A and C share nothing: both spend at once, and B's keys enter nothing
        keys = M.abc(b"abc2")
        assert b.spend(keys, 2, [True, False, True]) == ([0, 1, 0], [0, 0, 0], 1)
        assert b.order[-4:] == keys[0:2] + keys[4:6]
        assert b.spend(keys[2:4], 2) == ([M.SPENT_STORED], [0], 0)  # B itself, later: its n2 is A's by now
    finally:
        b.close()


def test_reason_follows_key_order_not_round_order(ctx):
    """transfer 4 is refused in round 2 over its key 1, but its key 0 fails too
    (spent by transfer 3, accepted in round 3): the verdict names key 0's owner"""
    for pad in (0, 130):  # alone (one workgroup), and behind 130 unrelated transfers (launch pairs)
        b = Both(ctx, 1024)
        try:
            front = [M.key(i, b"pad") for i in range(2 * pad)]
            v, d, rounds = b.spend(front + M.reasons_pile(), 2)
            assert v[pad:] == [0, 0, 3, 0, 3] and d[pad:] == [0, 0, pad + 1, 0, pad + 3] and rounds == 3
            # stored beats spent-in-call beats repeated, per key; the first failing key decides
            a, f = M.reasons_pile()[0], M.reasons_pile()[8]
            x, y = M.key(1, b"new"), M.key(2, b"new")
            pile = [x, y, y, a, x, x, f, y]  # t0 fresh; t1 {y: t0's, a: stored}; t2 {x: t0's, x}; t3 {f: stored, y}
            assert b.spend(pile, 2)[:2] == ([0, 3, 3, 2], [0, 0, 0, 0])
            z = M.key(3, b"new")
            assert b.spend([z, z, a], 3)[:2] == ([M.DUP_IN_TX], [1])  # z, z repeats (key 1) before a is looked at
            assert b.spend([z, a, z], 3)[:2] == ([M.SPENT_STORED], [1])
        finally:
            b.close()


# ------------------------------------------- 2b. more blocks than the scan has lanes
def test_block_offsets_with_a_run_of_two_blocks_a_lane(ctx):
    """65,537 transfers are 257 blocks of 256, one more than the one-workgroup
    prefix sum over the blocks' accepted counts has lanes (lane_util.h
    k_block_offsets<256>): a lane sums a run of two blocks, lane 128 a run of
    one, and the lanes behind it clamp to an empty run.  Transfers 255 / 256
    (the last lane of block 0, the first of block 1) share a key, and so do 0 /
    65,536 (the lone transfer of block 256): the later of each pair is refused
    with the earlier as its detail, so blocks 1 and 256 count one less than
    their lanes and every offset behind block 1 depends on it.  Verdicts,
    details, count and the log's order against the sequential model."""
    from zelana_amd import gpu
    n = 256 * 256 + 1
    keys = [M.key(i, b"wide") for i in range(n)]
    keys[n - 1], keys[256] = keys[0], keys[255]
    stored, order = set(), []
    want_v, want_d = M.spend(stored, order, keys, 1)
    assert (want_v[256], want_d[256]) == (M.SPENT_IN_CALL, 255)
    assert (want_v[n - 1], want_d[n - 1]) == (M.SPENT_IN_CALL, 0)
    assert want_v.count(M.ACCEPTED) == n - 2 == len(order)
    s = gpu.NullifierSetDevice(ctx, 1 << 17)
    try:
        v, d, _ = s.spend(keys, 1)
        bad = [t for t in range(n) if (v[t], d[t]) != (want_v[t], want_d[t])]
        assert not bad, (bad[:5], [(v[t], d[t], want_v[t], want_d[t]) for t in bad[:5]])
        assert s.count == len(order)
        log = s.log(0, s.count)
        bad = [i for i in range(len(order)) if log[i] != order[i]]
        assert not bad, ("the log's order", bad[:5])
    finally:
        s.close()


# ------------------------------------------------- 3. a small table, to the brim
def test_capacity_16_wraps_shares_a_home_slot_and_refuses(ctx):
    b = Both(ctx, 16)
    try:
        assert b.raw.info() == [16, 32, 0]
        crowd = M.keys_with_home(32, 30, 7)  # slots 30, 31, then across the table's end
        assert len({M.slot(k, 32) for k in crowd}) == 1
        other = [M.key(i, b"fill") for i in range(40)]
        b.spend(crowd[:6] + other[:2], 2)
        b.check_state(crowd + other[:4])
        b.spend(other[2:10], 1)  # exactly 16
        assert b.raw.info()[2] == 16
        b.check_state(crowd + other[:12])
        probes = crowd + other[:24]
        assert b.spend([crowd[6]], 1) is None  # one more key
        assert b.spend(other[10:12], 2) is None
        # the first transfer is refused (stored), the second alone overflows: the pile is refused whole
        assert b.spend([other[0], other[20], other[21], other[22]], 2) is None
        assert b.raw.info() == [16, 32, 16]
        b.check_state(probes)
        # refusals that add nothing still go through on the full set
        assert b.spend([other[0], other[20], crowd[1], crowd[6]], 2)[:2] == ([2, 2], [0, 0])
        b.check_state(probes)
    finally:
        b.close()


# ------------------------------------------------------------------- 4. the log
def test_log_is_insertion_order_across_calls(ctx):
    b = Both(ctx, 64)
    try:
        k = [M.key(i, b"log") for i in range(12)]
        b.spend(k[0:6], 3)
        b.spend([k[6], k[0], k[7], k[8], k[9], k[10]], 2, [True, True, True])  # the first transfer is refused
        assert b.order == k[0:6] + k[7:11]
        rc, got = b.raw.log(4, 5)
        assert rc == 0 and got == b.order[4:9]
        assert b.raw.log(10, 0)[0] == 0 and b.raw.log(0, 0)[0] == 0
        for first, n in ((10, 1), (11, 0), (0, 11), (2 ** 40, 1)):
            assert b.raw.log(first, n)[0] == EINVAL, (first, n)
    finally:
        b.close()


def test_load_collapses_duplicates(ctx):
    from zelana_amd import gpu
    s = gpu.NullifierSetDevice(ctx, 32)
    try:
        k = [M.key(i, b"load") for i in range(5)]
        v, d, _ = s.load([k[0], k[1], k[0], k[2], k[1], k[3]])
        assert v == [0, 0, 3, 0, 3, 0] and d == [0, 0, 0, 0, 1, 0]
        assert s.count == 4 and s.log(0, 4) == k[:4]
        assert s.contains(k) == [True] * 4 + [False]
        assert s.spend([], 2) == ([], [], 0)
    finally:
        s.close()


# -------------------------------------------------------- 5. argument errors
def test_argument_errors(ctx):
    from zelana_amd._lib import lib, vp
    from zelana_amd.gpu import Context
    L = lib()
    h = vp()
    assert L.zkmi_nullifier_set_create(ctx.h, 0, ctypes.byref(h)) == EINVAL
    assert L.zkmi_nullifier_set_create(ctx.h, 2 ** 31 + 1, ctypes.byref(h)) == EINVAL
    assert not h
    r = Raw(ctx, 8)
    other = Context(0)
    try:
        k = [M.key(i, b"arg") for i in range(5)]
        assert r.spend(k[:1], 1, [True])[:2] == (0, [0])
        for per_tx in (0, 5):
            v = np.full(4, FILL32, np.uint32)
            rc = L.zkmi_nullifier_set_spend(ctx.h, r.h, 1, per_tx, _u8(_kb(k)), None, _u32(v), _u32(v), None)
            assert rc == EINVAL and (v == FILL32).all()
        # ntx = 0 and n = 0 succeed and touch nothing, null pointers and all
        assert L.zkmi_nullifier_set_spend(ctx.h, r.h, 0, 2, None, None, None, None, None) == 0
        assert L.zkmi_nullifier_set_contains(ctx.h, r.h, 0, None, None) == 0
        # a set of another context
        out = np.full(4, FILL8, np.uint8)
        assert L.zkmi_nullifier_set_contains(other.h, r.h, 1, _u8(_kb(k)), _u8(out)) == EINVAL
        v = np.full(4, FILL32, np.uint32)
        assert L.zkmi_nullifier_set_spend(other.h, r.h, 1, 1, _u8(_kb(k[1:])), None, _u32(v), _u32(v), None) == EINVAL
        assert L.zkmi_nullifier_set_log(other.h, r.h, 0, 1, _u8(out)) == EINVAL
        assert (out == FILL8).all() and (v == FILL32).all()
        assert r.info() == [8, 16, 1] and r.contains(k[:2]) == [True, False]
    finally:
        other.close()
        r.close()


# -------------------------------------------------------------- 6. whole keys
def test_keys_equal_in_one_half_are_distinct(ctx):
    b = Both(ctx, 32)
    try:
        lo, hi = M.halves()
        assert len({k[:16] for k in lo}) == 1 and len({k[16:] for k in hi}) == 1
        assert b.spend(lo + hi, 2)[:2] == ([0, 0, 0], [0, 0, 0])
        cross = lo[0][:16] + hi[0][16:]
        b.check_state(lo + hi + [cross])
        assert b.spend([cross, lo[1]], 1)[0] == [M.ACCEPTED, M.SPENT_STORED]
    finally:
        b.close()
