"""ShieldedPool.settle with encrypted output notes and ShieldedPool.scan: a
small honest pile plus one refused transfer through one pool, every note
encrypted by the plain-Python model (zelana_amd/note_crypt.py); each
recipient's scan must return exactly their notes of the ACCEPTED transfers, at
the positions their commitments received.  The same pile through a second pool
without the keyword gives the same Settlements and stores nothing."""
import pytest

import note_crypt_cases as C
from zelana_amd import note_crypt as NC

pytestmark = pytest.mark.gpu

DEPTH = 4


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


def b(v):
    return bytes([v] * 32)


def test_settle_stores_the_accepted_notes_and_scan_finds_them(ctx):
    from zelana_amd import gpu, shielded as S, shielded_pool as SP
    fmt = gpu.PROOF_ARK_COMPRESSED
    sp = S.ShieldedProver(ctx, (DEPTH, DEPTH, 2), seed=3)
    pools = [SP.ShieldedPool(ctx, sp, depth=DEPTH, capacity=16, nullifier_capacity=16, empty_leaf=0, max_ct=100)
             for _ in range(2)]
    try:
        pool = pools[0]
        h = pool.tree.hasher
        specs = [(100 + 10 * i, b(10 + i), b(20 + i), i) for i in range(4)]
        notes = pool.tree.spend_notes(specs)
        pools[1].tree.spend_notes(specs)
        # three recipients: an X25519 key to decrypt with, an owner key inside the commitment
        sks = [C.rnd(f"pool/sk/{i}") for i in range(3)]
        xpk = [NC.public_key(sk) for sk in sks]
        owner = [b(40), b(41), b(42)]
        to = [[0, 1], [2, 0]]  # recipients of A's and of B's outputs
        values = [[150, 47], [200, 17]]
        memos = [[b"rent", None], ["café".encode(), b"\xff\xfe"]]
        outs = [[S.OutputNote(values[t][k], b(30 + 2 * t + k), owner[to[t][k]]) for k in range(2)] for t in range(2)]
        A, B = S.honest_many(h, [notes[0:2], notes[2:4]], outs, tree=pool.tree)
        pA, pB = sp.prove_many([A, B], [11, 12])

        def pub(t):
            return [t.merkle_root] + list(t.nullifiers) + list(t.commitments) + [S._b32(t.fee)]

        def enc(t, tag):
            return [NC.encrypt_note(values[t][k], b(30 + 2 * t + k), xpk[to[t][k]], memos[t][k],
                                    esk=C.rnd(f"pool/esk/{tag}/{k}"), nonce=C.rnd(f"pool/n/{tag}/{k}", 12))
                    for k in range(2)]

        pile = [(pub(A), pA.compressed(), enc(0, "A")), (pub(B), pB.compressed(), enc(1, "B")),
                (pub(A), pA.compressed(), enc(0, "again"))]  # the third repeats A: refused, its notes stored nowhere
        pubs, raws, encs = ([x[i] for x in pile] for i in range(3))
        got = pool.settle(fmt, raws, pubs, encrypted_notes=encs)
        assert [s.status for s in got] == ["ACCEPTED", "ACCEPTED", "SPENT_IN_CALL"]
        assert got[0].positions == [4, 5] and got[1].positions == [6, 7]
        plain = pools[1].settle(fmt, raws, pubs)
        assert plain == got, "the keyword changes no verdict, position or root"
        assert pools[1]._notes is None and pools[1].scan(sks[0], owner[0]) == ([], 0, [0, 0, 0, 0])

        assert pool.notes.info()[2:] == (4, sum(len(e[2]) for e in encs[0] + encs[1]))
        stored = pool.notes.get()
        assert [n[0] for n in stored] == [4, 5, 6, 7]
        assert [n[1] for n in stored] == [SP._b32(c) for c in list(A.commitments) + list(B.commitments)]
        assert [n[2:] for n in stored] == encs[0] + encs[1]

        want = {0: [(4, 150, b(30), "rent"), (7, 17, b(33), None)],   # a memo that is not UTF-8 comes back as None
                1: [(5, 47, b(31), None)],
                2: [(6, 200, b(32), "café")]}
        for r in range(3):
            hits, scanned_to, stats = pool.scan(sks[r], owner[r])
            assert [(x.position, x.value, x.randomness, x.memo) for x in hits] == want[r]
            assert [x.commitment for x in hits] == [stored[x.position - 4][1] for x in hits]
            assert scanned_to == 7 and stats == [4 - len(want[r]), 0, 0, len(want[r])]
            # the model's answer over what the store holds
            model = NC.scan_model(stored, sks[r], owner[r],
                                  lambda o, v, rnd: (S.note_commitment(v, rnd, o)).to_bytes(32, "little"))
            assert [(m[0], m[2], m[3]) for m in model[0]] == [(x.position, x.value, x.randomness) for x in hits]
        # pagination, the reference's MiMC scheme (these commitments are Poseidon's), the wrong owner key
        hits, scanned_to, _ = pool.scan(sks[0], owner[0], limit=1)
        assert [x.position for x in hits] == [4] and scanned_to == 4
        hits, scanned_to, _ = pool.scan(sks[0], owner[0], from_position=scanned_to + 1, limit=1)
        assert [x.position for x in hits] == [7] and scanned_to == 7
        assert pool.scan(sks[0], owner[0], scheme=SP.MIMC) == ([], 7, [2, 0, 2, 0])
        assert pool.scan(sks[0], owner[1])[2] == [2, 0, 2, 0]
        assert len(pool.scan(sks[0], owner[1], scheme=SP.NONE)[0]) == 2

        # shapes are checked before anything changes
        before = (pool.root(), pool.notes.count, pool.nullifiers.count)
        for bad in ([encs[0]], [encs[0][:1], encs[1], encs[0]], [[(b"", bytes(12), b"")] * 2] * 3,
                    [[(bytes(32), bytes(12), b"x" * 101)] * 2] * 3):
            with pytest.raises(ValueError):
                pool.settle(fmt, raws, pubs, encrypted_notes=bad)
        assert (pool.root(), pool.notes.count, pool.nullifiers.count) == before
    finally:
        for p in pools:
            p.close()
        sp.close()
