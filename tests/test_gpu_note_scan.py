"""The GPU-resident encrypted-note store and the batched note scan
(note_scan.hip over note_crypt.h; gpu.NoteStoreDevice above it) against the
plain-Python model (zelana_amd/note_crypt.py): first the per-op cases of
note_crypt_cases through a probe kernel (tests/device/note_crypt_probe.hip),
as the host check runs them on the CPU; then one pile of 257 notes, built and
classified once by the model, scanned as prefixes of 1, 63, 64, 65 and 257
notes (the wave and block edges of the compaction) under the three commitment
schemes, with from_position, limit and continued scans, several keys a call,
low-order and non-canonical ephemeral keys, and the store's refusals."""
import ctypes
import os
import random
import struct

import numpy as np
import pytest

import note_crypt_cases as C
from zelana_amd import note_crypt as NC
from zelana_amd.r1cs import R

pytestmark = pytest.mark.gpu

P = NC.P25519
SIZES = [1, 63, 64, 65, 257]
# ciphertext lengths of the notes addressed to key A that parse (memo = length - 58)
HIT_LENS = [58, 63, 64, 65, 80, 122, 123, 570]


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------- the probe
def test_per_op_cases_on_the_device():
    here = os.path.dirname(os.path.abspath(__file__))
    L = ctypes.CDLL(os.path.join(here, "..", "zelana_amd", "libzkmi_ncprobe.so"))
    assert (L.nc_probe_words(0), L.nc_probe_words(1)) == (C.NC_IN, C.NC_OUT)
    cases = C.all_cases()
    n = len(cases)
    ops = np.array([op for _, op, _, _ in cases], np.uint32)
    ins = np.zeros((n, C.NC_IN), np.uint32)
    for i, (_, _, w, _) in enumerate(cases):
        ins[i, :len(w)] = w
    out, nout = np.zeros((n, C.NC_OUT), np.uint32), np.zeros(n, np.int32)
    vp = ctypes.c_void_p
    L.nc_probe_run.argtypes = [ctypes.c_int, vp, vp, vp, vp]
    rc = L.nc_probe_run(n, ops.ctypes.data, ins.ctypes.data, out.ctypes.data, nout.ctypes.data)
    assert rc == 0, f"HIP error {rc}"
    assert (nout >= 0).all()
    C.check_outputs(cases, [out[i, :nout[i]].tolist() for i in range(n)])


# -------------------------------------------------------------------- the pile
def _mimc_commit(owner, value, rand):
    from zelana_amd.zbatch import mimc_hash
    le = lambda b: int.from_bytes(b, "little") % R
    return mimc_hash(le(owner), value % R, le(rand)).to_bytes(32, "little")


def _poseidon_commit(owner, value, rand):
    from zelana_amd.shielded import note_commitment
    return (note_commitment(value, rand, owner) % R).to_bytes(32, "little")


COMMIT = {0: None, 1: _mimc_commit, 2: _poseidon_commit}


class Pile:
    """257 notes in append order with shuffled, non-contiguous positions, and
    what the model says of every (key, note) pair under every scheme."""

    def __init__(self):
        rnd = C.rnd
        self.sks = [rnd("scan/sk/a"), rnd("scan/sk/b"), rnd("scan/sk/c")]  # c is sent nothing
        self.pks = [NC.public_key(sk) for sk in self.sks]
        self.owners = [rnd("scan/owner/a"), b"\xff" * 32, rnd("scan/owner/c")]  # b's is far above r
        n = SIZES[-1]
        positions = [3 * j + 1 for j in range(n)]
        random.Random(7).shuffle(positions)
        # what goes where: hits of A at the first and the last index of every prefix, the listed lengths, B's few
        plan = {0: ("hit", 0, 58, 2), 62: ("hit", 0, 58, 1), 63: ("hit", 0, 63, 2), 64: ("hit", 0, 64, 2),
                256: ("hit", 0, 570, 2), 100: ("hit", 0, 65, 1), 101: ("hit", 0, 80, 2), 102: ("hit", 0, 122, 2),
                103: ("hit", 0, 123, 1), 130: ("hit", 0, 570, 1), 131: ("hit", 0, 58, 2), 200: ("hit", 0, 59, 2),
                5: ("hit", 1, 58, 2), 70: ("hit", 1, 90, 2), 255: ("hit", 1, 64, 1),
                10: ("raw", 0), 11: ("raw", 15), 12: ("raw", 16), 13: ("tagged", 0, 16), 14: ("tagged", 0, 57),
                15: ("memo_len past the end", 0), 16: ("trailing", 0),
                20: ("epk", 0), 21: ("epk", 1), 22: ("epk", P - 1), 23: ("epk", P), 24: ("epk", P + 1),
                25: ("epk alias",), 26: ("epk bit255",)}
        self.notes = []
        for i in range(n):
            what = plan.get(i, ("foreign",))
            value, rand, cm = 1000 + i, rnd(f"scan/rand/{i}"), rnd(f"scan/cm/{i}")
            nonce = rnd(f"scan/nonce/{i}", 12)
            if what[0] == "hit":
                _, k, ct_len, scheme = what
                memo = rnd(f"scan/memo/{i}", ct_len - 58) if i != 200 else b"\xc3"  # one byte that is not UTF-8
                epk, nonce, ct = NC.encrypt_note(value, rand, self.pks[k], memo, esk=rnd(f"scan/esk/{i}"), nonce=nonce)
                cm = COMMIT[scheme](self.owners[k], value, rand)
                assert len(ct) == ct_len
            elif what[0] == "foreign" and i % 8 == 0:  # a real note to somebody else
                to = NC.public_key(rnd(f"scan/other/{i % 5}"))
                epk, nonce, ct = NC.encrypt_note(value, rand, to, rnd(f"scan/memo/{i}", i % 23), esk=rnd(f"scan/esk/{i % 9}"),
                                                 nonce=nonce)
            elif what[0] == "foreign":  # random bytes fail the tag as such a note does, and spare the model two ladders
                epk, ct = rnd(f"scan/fepk/{i}"), rnd(f"scan/fct/{i}", 58 + i % 23)
            elif what[0] == "raw":
                epk, ct = NC.public_key(rnd(f"scan/esk/{i}")), rnd(f"scan/raw/{i}", what[1])
            else:
                # made from the recipient's side, so any 32 bytes can stand as the ephemeral key
                if what[0] == "epk":
                    epk = what[1].to_bytes(32, "little")
                elif what[0] == "epk alias":  # p + 9: another encoding of the base point (only u < 19 has one)
                    epk = (P + 9).to_bytes(32, "little")
                elif what[0] == "epk bit255":
                    epk = (int.from_bytes(NC.public_key(rnd("scan/b255")), "little") | 1 << 255).to_bytes(32, "little")
                else:
                    epk = NC.public_key(rnd(f"scan/esk/{i}"))
                key = NC.derive_note_key(NC.x25519(self.sks[0], epk), epk)
                head = struct.pack("<Q", value) + rand
                pt = {"tagged": (head + b"\0\0")[:what[2] - 16] if what[0] == "tagged" else None,
                      "memo_len past the end": head + struct.pack("<H", 6) + b"short",
                      "trailing": head + struct.pack("<H", 2) + b"okTRAILING"}.get(what[0], head + struct.pack("<H", 3) + b"epk")
                ct = NC.chacha20_poly1305_seal(key, nonce, pt)
                cm = _poseidon_commit(self.owners[0], value, rand)
            self.notes.append((positions[i], cm, epk, nonce, ct))
        assert {len(x[4]) for x in self.notes} >= {0, 15, 16, 57, *HIT_LENS}
        # the model, once: scheme 0 per pair, then the commitment of the pairs that parse
        self.table = {}
        for k in range(3):
            for i, (pos, cm, epk, nonce, ct) in enumerate(self.notes):
                res, got = NC.classify((epk, nonce, ct), self.sks[k], self.owners[k], cm)
                for scheme in (0, 1, 2):
                    r = res
                    if res == NC.HIT and scheme and COMMIT[scheme](self.owners[k], got[0], got[1]) != cm:
                        r = NC.WRONG_COMMITMENT
                    self.table[k, i, scheme] = (r, got)

    def expect(self, n, k, scheme, from_position=0, limit=1000):
        stats, hits, top = [0, 0, 0, 0], [], None
        for i, (pos, cm, *_) in enumerate(self.notes[:n]):
            if pos < from_position:
                continue
            top = pos if top is None else max(top, pos)
            r, got = self.table[k, i, scheme]
            stats[r] += 1
            if r == NC.HIT:
                hits.append((pos, cm, got[0], got[1], got[2]))
        hits.sort()
        if len(hits) > limit:
            hits = hits[:limit]
            return hits, hits[-1][0], stats
        return hits, from_position if top is None else top, stats


@pytest.fixture(scope="module")
def pile():
    p = Pile()
    # the model itself, on a prefix, against the table built from its pieces
    hits, to, stats = NC.scan_model(p.notes[:65], p.sks[0], p.owners[0], _poseidon_commit)
    assert (hits, to, stats) == p.expect(65, 0, 2)
    return p


@pytest.fixture(scope="module")
def hashers(ctx):
    from zelana_amd import gpu
    from zelana_amd.shielded import shielded_hasher
    m, p = gpu.MimcHasher(ctx), shielded_hasher(ctx)
    yield m, p
    m.close()
    p.close()


@pytest.fixture(scope="module")
def full(ctx, hashers, pile):
    from zelana_amd import gpu
    s = gpu.NoteStoreDevice(ctx, 300, 570, mimc=hashers[0], poseidon=hashers[1])
    s.append(pile.notes[:100])
    s.append(pile.notes[100:])
    yield s
    s.close()


def _flat(result):
    hits, to, stats = result
    return [(h.position, h.commitment, h.value, h.randomness, h.memo) for h in hits], to, stats


def test_the_pile_holds_what_the_cases_need(pile):
    want = pile.expect(257, 0, 2)
    assert want[2][NC.MALFORMED] == 3 and want[2][NC.WRONG_COMMITMENT] >= 4 and len(want[0]) >= 10
    assert pile.expect(257, 0, 1)[2][NC.WRONG_COMMITMENT] >= 8 and len(pile.expect(257, 0, 1)[0]) == 4
    assert sum(pile.expect(257, 0, 0)[2][1:]) == sum(want[2][1:])
    assert pile.expect(257, 2, 1)[0] == [] and pile.expect(257, 2, 2)[0] == []  # key c: no hit under a commitment check
    assert len(pile.expect(257, 2, 0)[0]) == 5, "the low-order ephemeral keys open under every key"
    for i in (20, 21, 22, 23, 24):
        assert NC.x25519(pile.sks[2], pile.notes[i][2]) == bytes(32)
    for n in SIZES:  # hits at the first and at the last index
        assert pile.table[0, 0, 0][0] == NC.HIT and pile.table[0, n - 1, 0][0] == NC.HIT
    order = [pile.notes[i][0] for i in range(257)]
    assert order != sorted(order) and len(set(order)) == 257


@pytest.mark.parametrize("n", SIZES)
def test_prefixes_under_every_scheme(ctx, hashers, pile, n):
    from zelana_amd import gpu
    from zelana_amd._lib import lib
    streams = lib().zkmi_ctx_stream_count(ctx.h)
    s = gpu.NoteStoreDevice(ctx, n, 570, mimc=hashers[0], poseidon=hashers[1])
    try:
        s.append(pile.notes[:n])
        assert s.info() == (n, 570, n, sum(len(x[4]) for x in pile.notes[:n]))
        assert s.get() == pile.notes[:n]
        for scheme in (0, 1, 2):
            got = s.scan(pile.sks, pile.owners, scheme)
            assert [_flat(g) for g in got] == [pile.expect(n, k, scheme) for k in range(3)], (n, scheme)
        # the store is full now
        with pytest.raises(Exception, match=r"\(-4\)"):
            s.append([(999999, bytes(32), bytes(32), bytes(12), b"x" * 58)])
        assert s.count == n
    finally:
        s.close()
    assert lib().zkmi_ctx_stream_count(ctx.h) == streams, "no call of the store opens a stream"


def test_from_position_limit_and_continued_scans(full, pile):
    mid = sorted(x[0] for x in pile.notes)[128]
    for scheme in (0, 2):
        got = full.scan(pile.sks[:2], pile.owners[:2], scheme, from_position=mid)
        assert [_flat(g) for g in got] == [pile.expect(257, k, scheme, mid) for k in range(2)]
        assert got[0][2] != pile.expect(257, 0, scheme)[2], "the cut takes notes out of the statistics"
    all_hits = pile.expect(257, 0, 2)[0]
    for limit in (1, len(all_hits) - 1, len(all_hits), len(all_hits) + 1):
        seen, start, calls = [], 0, 0
        while True:
            got = _flat(full.scan([pile.sks[0]], [pile.owners[0]], 2, from_position=start, limit=limit)[0])
            assert got == pile.expect(257, 0, 2, start, limit), (limit, start)
            seen += got[0]
            calls += 1
            if len(got[0]) < limit or got[1] == max(x[0] for x in pile.notes):
                break
            start = got[1] + 1
        assert seen == all_hits, "continued scans lose nothing and repeat nothing"
        if limit == 1:
            assert calls >= len(all_hits)
    # past the last position: nothing examined, scanned_to = from_position
    assert _flat(full.scan([pile.sks[0]], [pile.owners[0]], 2, from_position=10**6)[0]) == ([], 10**6, [0, 0, 0, 0])


def test_keys_in_one_call(full, pile):
    two = full.scan([pile.sks[1], pile.sks[2]], [pile.owners[1], pile.owners[2]], 1)
    assert [_flat(g) for g in two] == [pile.expect(257, 1, 1), pile.expect(257, 2, 1)]
    assert two[1][0] == [] and len(two[0][0]) == 1
    three = full.scan(pile.sks[::-1], pile.owners[::-1], 2)
    assert [_flat(g) for g in three] == [pile.expect(257, k, 2) for k in (2, 1, 0)]
    assert full.scan([], [], 2) == []
    # the same key under another owner: every commitment differs
    wrong = _flat(full.scan([pile.sks[0]], [pile.owners[2]], 2)[0])
    assert wrong[0] == [] and wrong[2][NC.WRONG_COMMITMENT] == sum(pile.expect(257, 0, 0)[2][2:])
    # without memos the notes are the same
    bare = full.scan([pile.sks[0]], [pile.owners[0]], 2, memos=False)[0]
    assert [(h.position, h.value) for h in bare[0]] == [(h[0], h[2]) for h in pile.expect(257, 0, 2)[0]]


def test_block_offsets_with_a_run_of_two_blocks_a_lane(ctx, hashers):
    """8,193 notes under 8 keys in one call are 33 x 8 = 264 blocks of 256
    pairs, more than the one-workgroup prefix sum over the blocks' flag counts
    has lanes (lane_util.h k_block_offsets<256>): a lane sums a run of two
    blocks and the lanes behind lane 131 clamp to an empty run.  The notes are
    random bytes but four real ones: store indices 0 and 256 (blocks 0 and 1
    of the first key: the two blocks of lane 0's run) to the first key, 255 and
    8,192 (blocks 231 and 263: the second block of another lane's run, and the
    last block of all) to the last key.  The model classifies the four real
    notes under every key and a sample of the others; the rest are NOT_MINE
    under every key as the sample is: the model opens a note only when its 16
    tag bytes match, which random bytes do with probability 2^-128."""
    from zelana_amd import gpu
    n, nk = 8193, 8
    rng = random.Random(8193)
    sks = [C.rnd(f"wide/sk/{k}") for k in range(nk)]
    owners = [C.rnd(f"wide/owner/{k}") for k in range(nk)]
    to = {0: 0, 255: nk - 1, 256: 0, n - 1: nk - 1}
    notes = []
    for i in range(n):
        if i in to:
            value, rand = 5000 + i, C.rnd(f"wide/rand/{i}")
            epk, nonce, ct = NC.encrypt_note(value, rand, NC.public_key(sks[to[i]]), b"memo %d" % i,
                                             esk=C.rnd(f"wide/esk/{i}"), nonce=C.rnd(f"wide/nonce/{i}", 12))
            notes.append((i, _poseidon_commit(owners[to[i]], value, rand), epk, nonce, ct))
        else:
            notes.append((i, rng.randbytes(32), rng.randbytes(32), rng.randbytes(12), rng.randbytes(58 + i % 7)))
    # the model: the real notes and a sample of the random ones under every key
    want = []
    for k in range(nk):
        part = [notes[i] for i in sorted(to)] + [notes[1 + 1000 * k]]
        hits, _, stats = NC.scan_model(part, sks[k], owners[k], _poseidon_commit)
        stats[NC.NOT_MINE] += n - len(part)
        want.append((hits, n - 1, stats))
    assert [len(w[0]) for w in want] == [2] + [0] * (nk - 2) + [2]
    assert all(w[2] == [n, 0, 0, 0] for w in want[1:-1]) and want[0][2] == want[-1][2] == [n - 2, 0, 0, 2]
    s = gpu.NoteStoreDevice(ctx, n, 80, mimc=hashers[0], poseidon=hashers[1])
    try:
        s.append(notes)
        assert [_flat(g) for g in s.scan(sks, owners, 2)] == want
    finally:
        s.close()


def test_refusals_leave_the_store_as_it_was(ctx, hashers, pile):
    from zelana_amd import gpu
    s = gpu.NoteStoreDevice(ctx, 8, 100)
    try:
        ok = [n for n in pile.notes[:40] if len(n[4]) <= 100][:4]
        s.append(ok)
        before = (s.info(), s.get())
        long_ct = (6, bytes(32), bytes(32), bytes(12), b"x" * 101)
        fresh = (9, bytes(32), bytes(32), bytes(12), b"y" * 58)
        for bad, code in (([fresh, long_ct], -1),                        # a ciphertext above max_ct
                          ([fresh, (9,) + fresh[1:]], -1),               # a position twice in one call
                          ([fresh, (ok[0][0],) + fresh[1:]], -1),        # a position stored by an earlier call
                          ([(300 + 3 * i,) + fresh[1:] for i in range(5)], -4)):  # five notes where four fit
            with pytest.raises(Exception, match=rf"\({code}\)"):
                s.append(bad)
            assert (s.info(), s.get()) == before
        s.append([fresh])
        assert s.count == 5 and s.get(4, 1) == [fresh] and s.get(1, 2) == ok[1:3]
        with pytest.raises(Exception, match=r"\(-1\)"):
            s.get(3, 3)
        # a scheme needs its hasher; limit and the number of keys are bounded
        for kw in (dict(scheme=1), dict(scheme=2), dict(scheme=3), dict(scheme=0, n=65)):
            with pytest.raises(Exception, match=r"\(-1\)"):
                s.scan([bytes(32)] * kw.get("n", 1), [bytes(32)] * kw.get("n", 1), kw["scheme"])
        with pytest.raises(ValueError):
            s.scan([bytes(32)], [bytes(32)], 0, limit=0)
        assert len(s.scan([bytes(32)] * 64, [bytes(32)] * 64, 0, limit=2)) == 64
    finally:
        s.close()
    for cap, max_ct in ((0, 570), (1 << 27, 570), (8, 57)):
        with pytest.raises(Exception, match=r"\(-1\)"):
            gpu.NoteStoreDevice(ctx, cap, max_ct)
