"""CPU: the plain-Python Ed25519 model (zelana_amd/ed25519.py) against
libcrypto's answers in tests/golden/ed25519_vectors.json (public keys and
signatures byte for byte, verdicts as ok / not ok, the reason against each
case's construction), the message builders against literal strings, and
tx_auth's reasons over the model."""
import hashlib

import pytest

import ed25519_cases as C
from zelana_amd import ed25519 as E
from zelana_amd import tx_auth as T


def test_public_keys_and_signatures_match_libcrypto():
    g = C.golden()["sign"]
    assert [c["len"] for c in g] == [0, 1, 47, 48, 63, 64, 65, 175, 176, 300]
    for c in g:
        seed, msg = bytes.fromhex(c["seed"]), bytes.fromhex(c["msg"])
        assert len(msg) == c["len"]
        assert E.public_key(seed).hex() == c["public_key"], c["len"]
        assert E.sign(seed, msg).hex() == c["signature"], c["len"]


def test_verdicts_match_libcrypto_and_the_construction():
    triples = C.golden_triples()
    assert len(triples) == 10 + 17
    for name, pk, msg, sig, ok, reason in triples:
        v = E.verify(pk, msg, sig)
        assert (v == E.SIG_OK) == ok, (name, "libcrypto's verdict", v)
        assert v == reason, (name, v, reason)


def test_key_is_judged_before_s():
    c = next(c for c in C.golden()["verify"] if c["name"] == "A not on the curve")
    pk, msg, sig = (bytes.fromhex(c[k]) for k in ("public_key", "msg", "signature"))
    assert E.verify(pk, msg, sig[:32] + C.le32(E.L)) == E.SIG_BAD_PUBKEY
    with pytest.raises(ValueError):
        E.verify(pk, msg, sig[:63])


FROM = bytes(range(32))
TO = bytes(range(32, 64))
U64 = 2**64 - 1


def test_transfer_messages_are_the_references_strings():
    assert E.transfer_message(FROM, TO, U64, 0, 1) == (
        b"Zelana L2 Transfer\n\n"
        b"From: 000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f\n"
        b"To: 202122232425262728292a2b2c2d2e2f303132333435363738393a3b3c3d3e3f\n"
        b"Amount: 18446744073709551615 lamports\n"
        b"Nonce: 0\n"
        b"Chain ID: 1\n\n"
        b"Sign to authorize this L2 transfer.")
    assert E.transfer_message(b"\xab" * 32, b"\xCD" * 32, 0, U64, U64) == (
        b"Zelana L2 Transfer\n\nFrom: " + b"ab" * 32 + b"\nTo: " + b"cd" * 32 + b"\nAmount: 0 lamports\n"
        b"Nonce: 18446744073709551615\nChain ID: 18446744073709551615\n\nSign to authorize this L2 transfer.")
    legacy = E.legacy_transfer_message(FROM, TO, 5, 0, U64)
    assert len(legacy) == 88
    assert legacy == FROM + TO + b"\x05" + bytes(7) + bytes(8) + b"\xff" * 8
    for bad in ((FROM[:31], TO, 1, 0, 1), (FROM, TO, 2**64, 0, 1), (FROM, TO, 1, -1, 1)):
        with pytest.raises(ValueError):
            E.transfer_message(*bad)


def test_withdraw_messages_are_the_references_strings():
    assert E.withdraw_message(FROM, bytes(32), U64, 0) == (
        b"Zelana L2 Withdrawal\n\n"
        b"From: 000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f\n"
        b"To L1: 11111111111111111111111111111111\n"
        b"Amount: 18446744073709551615 lamports\n"
        b"Nonce: 0\n\n"
        b"Sign to authorize this withdrawal to Solana L1.")
    # two leading zero bytes, then 0x01 0x00 ... 0x00 0xff: base58 keeps one '1' per leading zero byte
    to_l1 = bytes(2) + b"\x01" + bytes(28) + b"\xff"
    assert E.base58(bytes(2) + b"\x01") == "112" and E.base58(b"\xff") == "5Q" and E.base58(b"") == ""
    b58 = E.base58(to_l1)
    assert b58.startswith("11") and not b58.startswith("111")
    v = 0
    for ch in b58:  # decodes back, by the alphabet written out here
        v = v * 58 + "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz".index(ch)
    assert v == int.from_bytes(to_l1, "big")
    assert E.withdraw_message(FROM, to_l1, 7, 3) == (
        b"Zelana L2 Withdrawal\n\nFrom: 000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f\n"
        b"To L1: " + b58.encode() + b"\nAmount: 7 lamports\nNonce: 3\n\nSign to authorize this withdrawal to Solana L1.")
    # the Solana system program id and a well-known address, as published
    assert E.base58(bytes.fromhex("06ddf6e1d765a193d9cbe146ceeb79ac1cb485ed5f5b37913a8cf5857eff00a9")) == \
        "TokenkegQfeZyiNwAJbNbGKPFXCWuBvf9Ss623VQ5DA"
    legacy = E.legacy_withdraw_message(FROM, to_l1, U64, 1)
    assert len(legacy) == 80 and legacy == FROM + to_l1 + b"\xff" * 8 + b"\x01" + bytes(7)


def _seed(i):
    return hashlib.sha256(b"tx-auth-cpu/%d" % i).digest()


def test_tx_auth_reasons_over_the_model():
    mv = T.ModelVerifier()
    other = E.public_key(_seed(99))
    good = T.sign_transfer(_seed(0), TO, 5, 0, 1)
    legacy = T.sign_transfer(_seed(1), TO, 5, 0, 1, legacy=True)
    not_a_point = next(bytes.fromhex(c["public_key"]) for c in C.golden()["verify"] if c["name"] == "A not on the curve")
    bad_key = T.SignedTransfer(not_a_point, TO, 5, 0, 1, good.signature[:10], not_a_point)  # the key before the length
    short = T.SignedTransfer(good.from_, TO, 5, 0, 1, good.signature[:63], good.signer_pubkey)
    forged = T.SignedTransfer(good.from_, TO, 6, 0, 1, good.signature, good.signer_pubkey)
    big_s = T.SignedTransfer(good.from_, TO, 5, 0, 1, good.signature[:32] + C.le32(E.L), good.signer_pubkey)
    stolen = T.SignedTransfer(other, TO, 5, 0, 1, b"", E.public_key(_seed(2)))
    stolen.signature = E.sign(_seed(2), stolen.messages()[0])
    txs = [good, legacy, bad_key, short, forged, big_s, stolen]
    reasons, formats = T.verify_transfers(mv, txs)
    assert reasons == [T.OK, T.OK, T.INVALID_PUBKEY, T.INVALID_SIGNATURE_LENGTH, T.VERIFICATION_FAILED,
                       T.VERIFICATION_FAILED, T.FROM_MISMATCH]
    assert formats == [T.READABLE, T.LEGACY, None, None, None, None, T.READABLE]
    w = T.sign_withdrawal(_seed(3), bytes(32), 9, 4)
    wl = T.sign_withdrawal(_seed(3), bytes(32), 9, 5, legacy=True)
    wf = T.SignedWithdrawal(w.from_, bytes(32), 10, 4, w.signature, w.signer_pubkey)
    assert T.verify_withdrawals(mv, [w, wl, wf]) == ([T.OK, T.OK, T.VERIFICATION_FAILED], [T.READABLE, T.LEGACY, None])
    assert T.verify_transfers(mv, []) == ([], [])
    assert T.signature_field(bytes(range(64))) == int.from_bytes(bytes(range(31)), "big")
