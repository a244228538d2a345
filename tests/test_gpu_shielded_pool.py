"""ShieldedPool.settle on the GPU against a host model built from
shielded.NoteTree, a Python set and ShieldedProver.verify_each: two piles of
compressed proofs through one pool, with every kind of verdict in them.

Shape (4, 4, 2) over a depth-4 tree, not test_loop_closed_small's (3, 3, 2):
two accepted transfers of the first pile and two of the second put 8 output
commitments beside the 6 notes they spend, and a depth-3 tree holds 8 leaves."""
from collections import deque

import numpy as np
import pytest

from zelana_amd.r1cs import R

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


class Model:
    """the pool one transfer at a time on the host, with settle's two rules:
    non-canonical bytes are refused, roots are judged as the call finds the history"""

    def __init__(self, S):
        self.S, self.tree, self.next = S, S.NoteTree(DEPTH), 0
        self.history = deque([self.tree.root()], maxlen=S.ROOT_HISTORY_SIZE)
        self.spent, self.order = set(), []

    def insert(self, leaf):
        self.tree.insert(self.next, leaf)
        self.next += 1
        self.history.append(self.tree.root())
        return self.next - 1

    def settle(self, pile, n_in=2):
        """pile: (public inputs as 32-byte strings, proof verdict: True / False / "malformed")"""
        valid_roots = set(self.history)
        out = []
        owner = {}
        before = set(self.spent)
        for t, (pub, proof) in enumerate(pile):
            vals = [int.from_bytes(x, "little") for x in pub]
            nfs, cms = pub[1:1 + n_in], vals[1 + n_in:-1]
            if any(v >= R for v in vals):
                out.append(("NONCANONICAL", None, [], None))
            elif vals[0] not in valid_roots:
                out.append(("BAD_ROOT", None, [], None))
            elif proof is not True:
                out.append(("BAD_ENCODING" if proof == "malformed" else "BAD_PROOF", None, [], None))
            else:
                why = None
                for k, nf in enumerate(nfs):
                    if nf in before:
                        why = ("SPENT_STORED", k, [], None)
                    elif nf in owner:
                        why = ("SPENT_IN_CALL", owner[nf], [], None)
                    elif nf in nfs[:k]:
                        why = ("DUP_IN_TX", k, [], None)
                    if why:
                        break
                if why:
                    out.append(why)
                    continue
                for nf in nfs:
                    owner[nf] = t
                    self.spent.add(nf)
                    self.order.append(nf)
                pos = [self.insert(cm) for cm in cms]
                out.append(("ACCEPTED", None, pos, self.tree.root()))
        return out


def _tamper(gpu, raw, want_malformed):
    """raw with one byte of C's x changed so that it still decodes to a curve
    point (another, well-formed proof) or no longer decodes (malformed)"""
    for x in range(1, 256):
        cand = raw[:96] + bytes([raw[96] ^ x]) + raw[97:]
        try:
            gpu.proof_decode(gpu.PROOF_ARK_COMPRESSED, cand)
            malformed = False
        except gpu.ProofDecodeError as e:
            assert e.status == 1
            malformed = True
        if malformed == want_malformed:
            return cand
    raise AssertionError("no such byte")


def test_two_piles_through_one_pool(ctx):
    import zelana_amd
    from zelana_amd import gpu, shielded as S, shielded_pool as SP
    assert zelana_amd.ShieldedPool is SP.ShieldedPool and "ShieldedPool" in zelana_amd.__all__
    fmt = gpu.PROOF_ARK_COMPRESSED
    sp = S.ShieldedProver(ctx, (DEPTH, DEPTH, 2), seed=3)
    pool = SP.ShieldedPool(ctx, sp, depth=DEPTH, capacity=16, nullifier_capacity=16, empty_leaf=0)
    try:
        assert (pool.n_in, pool.n_out) == (2, 2)
        model = Model(S)
        h = pool.tree.hasher
        # six notes; A's outputs go to keys we hold, so the second pile can spend them
        specs = [(100 + 10 * i, b(10 + i), b(20 + i), i) for i in range(6)]
        notes = pool.tree.spend_notes(specs)
        for n in notes:
            model.insert(S.note_commitment(n.value, n.randomness, n.owner_pk))
        assert pool.root() == model.tree.root() and list(pool.tree.history) == list(model.history)
        fsk = [b(50), b(51)]
        fpk = [S._b32(v) for v in S.derive_pk_many(h, fsk)]
        outs = [[S.OutputNote(150, b(30), fpk[0]), S.OutputNote(57, b(31), fpk[1])],
                [S.OutputNote(200, b(32), b(42)), S.OutputNote(7, b(33), b(43))],
                [S.OutputNote(300, b(34), b(44)), S.OutputNote(3, b(35), b(45))]]
        A, B, T = S.honest_many(h, [notes[0:2], notes[2:4], notes[4:6]], outs, tree=pool.tree)
        pA, pB, pT = sp.prove_many([A, B, T], [11, 12, 13])
        rA, rB, rT = (p.compressed() for p in (pA, pB, pT))

        def pub(t):
            return [t.merkle_root] + list(t.nullifiers) + list(t.commitments) + [S._b32(t.fee)]

        bad_proof, malformed = _tamper(gpu, rT, False), _tamper(gpu, rT, True)
        never = pub(B)
        never[0] = S._b32(12345)  # canonical, and never a root
        alias = pub(T)
        alias[1] = (int.from_bytes(alias[1], "little") + R).to_bytes(32, "little")  # the honest nullifier plus r
        assert int.from_bytes(alias[1], "little") % R == S._fr_le(T.nullifiers[0])
        # the verdicts of the proofs as the host model takes them: verify_each on the decoded points
        dec = [gpu.proof_decode(fmt, r) for r in (rA, rB, bad_proof)]
        assert sp.verify_each([type(pA)(p.public_inputs, *d) for p, d in zip((pA, pB, pT), dec)]) == [True, True, False]

        pile1 = [(pub(A), rA, True), (pub(B), rB, True), (pub(A), rA, True), (pub(T), bad_proof, False),
                 (never, rB, True), (alias, rT, True), (pub(T), malformed, "malformed")]
        # public inputs as 32-byte strings for some transfers, as ints for others
        given = [x if i % 2 else [int.from_bytes(v, "little") for v in x] for i, (x, _, _) in enumerate(pile1)]
        got = pool.settle(fmt, [r for _, r, _ in pile1], given)
        want = model.settle([(x, ok) for x, _, ok in pile1])
        assert [(s.status, s.detail, s.positions, s.root) for s in got] == want
        assert [s.status for s in got] == ["ACCEPTED", "ACCEPTED", "SPENT_IN_CALL", "BAD_PROOF", "BAD_ROOT",
                                           "NONCANONICAL", "BAD_ENCODING"]
        assert got[2].detail == 0 and got[0].positions == [6, 7] and got[1].positions == [8, 9]
        assert got[0].accepted and not got[2].accepted

        def state():
            assert pool.root() == model.tree.root() and pool.tree.next_position == model.next
            assert list(pool.tree.history) == list(model.history)
            probes = A.nullifiers + B.nullifiers + T.nullifiers + [alias[1]]
            assert [pool.nullifier_exists(k) for k in probes] == [k in model.spent for k in probes]
            assert pool.spent_log() == model.order and pool.spent_log(1, 2) == model.order[1:3]
            return [pool.nullifier_exists(k) for k in T.nullifiers]

        assert state() == [False, False], "a refused transfer's nullifiers stay spendable"
        assert not pool.nullifier_exists(int.from_bytes(alias[1], "little"))

        # ---- the second pile: a replay, T as it was proven (its root is still recent), and a fresh
        # transfer over paths of the updated tree that spends A's outputs
        fresh = [S.InputNote(o.value, o.randomness, o.recipient_pk, p, sk) for o, p, sk in zip(outs[0], [6, 7], fsk)]
        for n, (sibs, bits) in zip(fresh, pool.paths([6, 7])):
            n.merkle_path, n.path_bits = sibs, bits
            assert (sibs, bits) == model.tree.path(n.position)
        F = S.honest_many(h, [fresh], [[S.OutputNote(200, b(36), b(46)), S.OutputNote(5, b(37), b(47))]],
                          tree=pool.tree)[0]
        assert S._fr_le(F.merkle_root) == model.tree.root() and F.fee == 2
        pF = sp.prove_many([F], [14])[0]
        pile2 = [(pub(B), rB, True), (pub(T), rT, True), (pub(F), pF.compressed(), True)]
        got = pool.settle(fmt, b"".join(r for _, r, _ in pile2), [x for x, _, _ in pile2], each=True)
        want = model.settle([(x, ok) for x, _, ok in pile2])
        assert [(s.status, s.detail, s.positions, s.root) for s in got] == want
        assert [(s.status, s.detail) for s in got] == [("SPENT_STORED", 0), ("ACCEPTED", None), ("ACCEPTED", None)]
        assert got[2].positions == [12, 13] and got[2].root == pool.root()
        assert state() == [True, True]
        assert pool.is_valid_root(A.merkle_root) and not pool.is_valid_root(12345)
        assert pool.settle(fmt, [], []) == []
    finally:
        pool.close()
        sp.close()


def test_key_and_shape_must_agree(ctx):
    """a pool over bare key bytes: the split of the public inputs is given, or half and half"""
    from zelana_amd import shielded as S, shielded_pool as SP
    sp = S.ShieldedProver(ctx, (1, 1), seed=1, precompute=False)  # one input, one output: 4 public inputs
    try:
        pool = SP.ShieldedPool(ctx, sp.verifying_key, depth=2, capacity=4, nullifier_capacity=4, empty_leaf=0)
        assert (pool.n_in, pool.n_out) == (1, 1)
        with pytest.raises(ValueError):
            pool.settle(0, [bytes(128)], [[0, 0, 0]])  # three public inputs where the key has four
        pool.close()
        with pytest.raises(ValueError):
            SP.ShieldedPool(ctx, sp.verifying_key, depth=2, capacity=4, nullifier_capacity=4, n_in=2, n_out=2)
    finally:
        sp.close()
