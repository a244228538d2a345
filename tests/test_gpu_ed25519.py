"""Batched Ed25519 verification on the GPU (ed25519.hip over ed25519.h;
gpu.Ed25519Verifier, tx_auth and DeviceAccountState.batches(verifier=) above
it) against the plain-Python model (zelana_amd/ed25519.py) and libcrypto's
golden verdicts: first the per-op cases of ed25519_cases through a probe kernel
(tests/device/ed25519_probe.hip), as the host check runs them on the CPU; then
verify_many at 1, 63, 64, 65 and 257 signatures with message lengths that
differ from lane to lane and every golden edge case at the wave's edges; the
ABI's edges; tx_auth over about 40 signed transactions; and signed batches
through the account state."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import ed25519_cases as C
from zelana_amd import ed25519 as E
from zelana_amd import tx_auth as T

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257]
MSG_LENS = [0, 47, 48, 63, 64, 65, 175, 176, 300]


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def verifier(ctx):
    from zelana_amd.gpu import Ed25519Verifier
    return Ed25519Verifier(ctx)


# ------------------------------------------------------------------- the probe
def test_per_op_cases_on_the_device():
    here = os.path.dirname(os.path.abspath(__file__))
    L = ctypes.CDLL(os.path.join(here, "..", "zelana_amd", "libzkmi_edprobe.so"))
    assert (L.ed_probe_words(0), L.ed_probe_words(1)) == (C.ED_IN, C.ED_OUT)
    cases = C.all_cases()
    n = len(cases)
    ops = np.array([op for _, op, _, _ in cases], np.uint32)
    ins = np.zeros((n, C.ED_IN), np.uint32)
    for i, (_, _, w, _) in enumerate(cases):
        ins[i, :len(w)] = w
    out, nout = np.zeros((n, C.ED_OUT), np.uint32), np.zeros(n, np.int32)
    vp = ctypes.c_void_p
    L.ed_probe_run.argtypes = [ctypes.c_int, vp, vp, vp, vp]
    rc = L.ed_probe_run(n, ops.ctypes.data, ins.ctypes.data, out.ctypes.data, nout.ctypes.data)
    assert rc == 0, f"HIP error {rc}"
    assert (nout >= 0).all()
    C.check_outputs(cases, [out[i, :nout[i]].tolist() for i in range(n)])


# -------------------------------------------------------------------- the pile
class Pile:
    """257 (public key, message, signature) triples and the model's verdict on
    each, made once: honest signatures over messages whose lengths cycle
    through MSG_LENS, every fifth one spoiled in a way of its own, and the
    golden edge cases, which prefix(n) places at lanes 0, 63, 64 and n - 1."""

    def __init__(self):
        self.edge = [(pk, msg, sig, reason) for _, pk, msg, sig, _, reason in C.golden_triples()]
        keys = [(s, E.public_key(s)) for s in (C.rnd(f"pile/seed/{j}") for j in range(6))]
        self.base = []
        for i in range(SIZES[-1]):
            seed, pk = keys[i % len(keys)]
            msg = C.rnd(f"pile/msg/{i}", MSG_LENS[i % len(MSG_LENS)])
            sig = E.sign(seed, msg)
            if i % 5 == 4:
                how = (i // 5) % 4
                if how == 0:
                    msg = msg + b"x"
                elif how == 1:
                    sig = sig[:32] + C.le32(int.from_bytes(sig[32:], "little") + E.L)
                elif how == 2:
                    sig = bytes([sig[0] ^ 1]) + sig[1:]
                else:
                    pk = C.le32(2)  # on no point
            self.base.append((pk, msg, sig, E.verify(pk, msg, sig)))
        assert {v for *_, v in self.base} == {0, 1, 2, 3}

    def prefix(self, n: int, round_: int):
        """the first n triples, with golden edge cases (a different four each
        round) at lanes 0, 63, 64 and n - 1"""
        out = list(self.base[:n])
        for j, lane in enumerate(sorted({0, 63, 64, n - 1})):
            if lane < n:
                out[lane] = self.edge[(4 * round_ + j) % len(self.edge)]
        return out


@pytest.fixture(scope="module")
def pile():
    return Pile()


def _run(verifier, triples):
    got = verifier.verify_many([t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples])
    assert got.dtype == np.uint8 and got.shape == (len(triples),)
    return got.tolist()


def test_verify_many_matches_the_model_at_every_size(verifier, pile):
    for n in SIZES:
        for round_ in range(1 if n < 64 else 3):  # other golden cases at the edge lanes each round
            triples = pile.prefix(n, round_ + 3 * SIZES.index(n))
            want = [t[3] for t in triples]
            got = _run(verifier, triples)
            assert got == want, (n, round_, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])


def test_every_golden_case_at_lanes_0_63_64_and_last(verifier, pile):
    n = 65 + len(pile.edge)
    for k, edge in enumerate(pile.edge):
        triples = list(pile.base[:n])
        for lane in (0, 63, 64, n - 1):
            triples[lane] = edge
        got = _run(verifier, triples)
        assert got == [t[3] for t in triples], (k, edge[3])


def test_all_good_and_all_bad_batches(verifier, pile):
    good = [t for t in pile.base if t[3] == E.SIG_OK][:70]
    assert _run(verifier, good) == [E.SIG_OK] * 70
    bad = [t for t in pile.base if t[3] != E.SIG_OK] + [e for e in pile.edge if e[3] != E.SIG_OK]
    assert len(bad) > 52
    assert _run(verifier, bad) == [t[3] for t in bad]
    assert E.SIG_OK not in [t[3] for t in bad]


# --------------------------------------------------------------------- the ABI
def test_abi_edges(ctx, verifier, pile):
    from zelana_amd._lib import ZkmiError, lib, u64p, u8p
    assert verifier.verify_many([], [], []).shape == (0,)
    # n = 0 with null arrays does nothing
    assert lib().zkmi_ed25519_verify_many(ctx.h, 0, None, None, None, None, None) == 0
    triples = pile.base[:3]
    pk = np.frombuffer(b"".join(t[0] for t in triples), np.uint8)
    sg = np.frombuffer(b"".join(t[2] for t in triples), np.uint8)
    ms = np.frombuffer(b"".join(t[1] for t in triples) + b"\0", np.uint8)
    lens = [len(t[1]) for t in triples]
    good = np.array([0, lens[0], lens[0] + lens[1], sum(lens)], np.uint64)
    assert verifier.verify_arrays(pk, sg, ms, good).tolist() == [t[3] for t in triples]
    out = np.full(3, 77, np.uint8)
    for bad in (np.array([0, 48, 47, 111], np.uint64), np.array([1, 1, 48, 111], np.uint64)):
        rc = lib().zkmi_ed25519_verify_many(ctx.h, 3, pk.ctypes.data_as(u8p), sg.ctypes.data_as(u8p), ms.ctypes.data_as(u8p),
                                            bad.ctypes.data_as(u64p), out.ctypes.data_as(u8p))
        assert rc == -1 and out.tolist() == [77] * 3  # ZKMI_EINVAL, nothing written
    with pytest.raises(ZkmiError):
        verifier.verify_arrays(pk, sg, ms, np.array([0, 48, 47, 95], np.uint64))
    with pytest.raises(ValueError):
        verifier.verify_many([b"\0" * 31], [b""], [b"\0" * 64])
    # two calls of different n on one context: the workspace of the larger call serves the smaller one after it
    big, small = pile.prefix(257, 1), pile.prefix(5, 2)
    assert _run(verifier, small) == [t[3] for t in small]
    assert _run(verifier, big) == [t[3] for t in big]
    assert _run(verifier, small) == [t[3] for t in small]


# --------------------------------------------------------------------- tx_auth
def _seed(i):
    return hashlib.sha256(b"tx-auth-gpu/%d" % i).digest()


def _forty_transfers():
    seeds = [_seed(i) for i in range(8)]
    pks = [E.public_key(s) for s in seeds]
    txs, want = [], []
    for i in range(34):
        legacy = i % 3 == 2
        txs.append(T.sign_transfer(seeds[i % 8], pks[(i + 1) % 8], 1000 + i, i, 1 + i % 2, legacy=legacy))
        want.append((T.OK, T.LEGACY if legacy else T.READABLE))
    g = txs[0]
    not_a_point = C.le32(2)
    txs.append(T.SignedTransfer(not_a_point, g.to, 5, 0, 1, g.signature[:10], not_a_point))
    want.append((T.INVALID_PUBKEY, None))
    txs.append(T.SignedTransfer(g.from_, g.to, g.amount, g.nonce, g.chain_id, g.signature + b"\0", g.signer_pubkey))
    want.append((T.INVALID_SIGNATURE_LENGTH, None))
    txs.append(T.SignedTransfer(g.from_, g.to, g.amount + 1, g.nonce, g.chain_id, g.signature, g.signer_pubkey))
    want.append((T.VERIFICATION_FAILED, None))
    txs.append(T.SignedTransfer(g.from_, g.to, g.amount, g.nonce, g.chain_id, g.signature[:32] + C.le32(E.L), g.signer_pubkey))
    want.append((T.VERIFICATION_FAILED, None))
    for legacy in (False, True):  # a valid signature by a key that is not `from`
        t = T.SignedTransfer(pks[3], pks[4], 9, 9, 1, b"", pks[5])
        t.signature = E.sign(seeds[5], t.messages()[1 if legacy else 0])
        txs.append(t)
        want.append((T.FROM_MISMATCH, T.LEGACY if legacy else T.READABLE))
    return txs, want


def test_verify_transfers_reasons_and_formats(verifier):
    txs, want = _forty_transfers()
    assert len(txs) == 40
    reasons, formats = T.verify_transfers(verifier, txs)
    assert list(zip(reasons, formats)) == want
    assert (reasons, formats) == T.verify_transfers(T.ModelVerifier(), txs)


def test_verify_withdrawals_reasons_and_formats(verifier):
    seeds = [_seed(100 + i) for i in range(5)]
    l1s = [bytes(32), bytes(3) + C.rnd("l1/a", 29), C.rnd("l1/b"), b"\xff" * 32]
    reqs, want = [], []
    for i in range(36):
        legacy = i % 4 == 3
        reqs.append(T.sign_withdrawal(seeds[i % 5], l1s[i % 4], 2**64 - 1 - i, i, legacy=legacy))
        want.append((T.OK, T.LEGACY if legacy else T.READABLE))
    g = reqs[0]
    reqs.append(T.SignedWithdrawal(C.le32(2), g.to_l1_address, 1, 0, b"", C.le32(2)))
    want.append((T.INVALID_PUBKEY, None))
    reqs.append(T.SignedWithdrawal(g.from_, g.to_l1_address, g.amount, g.nonce, b"", g.signer_pubkey))
    want.append((T.INVALID_SIGNATURE_LENGTH, None))
    reqs.append(T.SignedWithdrawal(g.from_, l1s[2], g.amount, g.nonce, g.signature, g.signer_pubkey))
    want.append((T.VERIFICATION_FAILED, None))
    w = T.SignedWithdrawal(E.public_key(seeds[1]), l1s[1], 4, 4, b"", E.public_key(seeds[2]))
    w.signature = E.sign(seeds[2], w.messages()[0])
    reqs.append(w)
    want.append((T.FROM_MISMATCH, T.READABLE))
    assert len(reqs) == 40
    reasons, formats = T.verify_withdrawals(verifier, reqs)
    assert list(zip(reasons, formats)) == want


# ----------------------------------------------------------- the account state
def test_signed_batches_through_the_account_state(ctx, verifier):
    from zelana_amd.account_state import DeviceAccountState
    # four keys with distinct leading bytes: a depth-8 tree places an account by the first byte of its id
    seeds, i = [], 200
    while len(seeds) < 4:
        if E.public_key(_seed(i))[0] not in {E.public_key(s)[0] for s in seeds}:
            seeds.append(_seed(i))
        i += 1
    ids = [E.public_key(s) for s in seeds]

    def signed_batches(forge: bool):
        b1 = {"batch_id": 7, "transfers": [T.sign_transfer(seeds[0], ids[1], 30, 0, 1),
                                            T.sign_transfer(seeds[1], ids[2], 5, 0, 1, legacy=True)],
              "withdrawals": [T.sign_withdrawal(seeds[2], C.rnd("acct/l1"), 11, 0)]}
        t = T.sign_transfer(seeds[0], ids[3], 8, 1, 1)
        if forge:
            t.amount = 80
        b2 = {"batch_id": 8, "transfers": [T.sign_transfer(seeds[3], ids[0], 2, 0, 1), t],
              "withdrawals": [T.sign_withdrawal(seeds[1], bytes(32), 3, 1, legacy=True)]}
        return [b1, b2]

    def fresh():
        st = DeviceAccountState(ctx, depth=8, max_nodes=1 << 12)
        st.insert_many([(i, 1000 + k, 0) for k, i in enumerate(ids)])
        return st

    honest = signed_batches(False)
    as_tuples = [{"batch_id": b["batch_id"], "transfers": [T.transfer_tuple(t) for t in b["transfers"]],
                  "withdrawals": [T.withdrawal_tuple(w) for w in b["withdrawals"]]} for b in honest]
    a, b = fresh(), fresh()
    try:
        want = a.batches(as_tuples)
        got = b.batches(honest, verifier=verifier)
        assert got == want
        assert b.root() == a.root() and b.accounts == a.accounts
        assert got[0]["transfers"][0]["signature"] == T.signature_field(honest[0]["transfers"][0].signature)
        # a forged signature in the second batch: refused before anything changes
        root, accounts = b.root(), {k: list(v) for k, v in b.accounts.items()}
        with pytest.raises(ValueError, match=r"batch 8: transfers\[1\] refused: signature verification failed"):
            b.batches(signed_batches(True), verifier=verifier)
        assert b.root() == root and b.accounts == accounts
        with pytest.raises(ValueError, match="need a verifier"):
            b.batches(honest)
        assert b.root() == root and b.accounts == accounts
    finally:
        a.close()
        b.close()
