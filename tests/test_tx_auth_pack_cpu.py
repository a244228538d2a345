"""CPU: tx_auth.pack, which turns SignedTransfer / SignedWithdrawal objects
into the fixed-width records of the device path (gpu.SIGNED_TX_DTYPE, the C
ABI's zkmi_signed_tx), and the dispatch between the two paths of tx_auth."""
import hashlib

import numpy as np
import pytest

from zelana_amd import ed25519 as E
from zelana_amd import gpu
from zelana_amd import tx_auth as T

SEED = hashlib.sha256(b"tx-auth-pack").digest()


def test_record_layout_is_the_abi_struct():
    d = gpu.SIGNED_TX_DTYPE
    assert d.itemsize == 192
    assert [d.fields[k][1] for k in ("from", "to", "amount", "nonce", "chain_id", "signer_pubkey", "signature", "kind",
                                     "reserved")] == [0, 32, 64, 72, 80, 88, 120, 184, 185]


def test_pack_lays_the_fields_out_and_refuses_what_the_host_path_refuses():
    g = T.sign_transfer(SEED, bytes(range(32)), 10**19, 2**64 - 1, 3)
    w = T.sign_withdrawal(SEED, bytes(31) + b"\x07", 5, 6, legacy=True)
    short = T.SignedWithdrawal(w.from_, w.to_l1_address, 5, 6, w.signature[:63], w.signer_pubkey)
    rec = T.pack([g, w, short])
    assert rec.dtype == gpu.SIGNED_TX_DTYPE and rec.shape == (3,)
    assert rec["kind"].tolist() == [gpu.TX_TRANSFER, gpu.TX_WITHDRAWAL, gpu.TX_WITHDRAWAL]
    assert rec["chain_id"].tolist() == [3, 0, 0] and not rec["reserved"].any()
    assert rec["from"][0].tobytes() == g.from_ and rec["signer_pubkey"][1].tobytes() == w.signer_pubkey
    assert rec["signature"][0].tobytes() == g.signature and rec["signature"][2].tobytes() == bytes(64)
    # the first 88 / 80 bytes of a record are its legacy message
    raw = rec.tobytes()
    assert raw[:88] == g.messages()[1] and raw[192:192 + 80] == w.messages()[1]
    assert T.pack([]).shape == (0,)
    for field, value in (("amount", 2**64), ("nonce", -1), ("chain_id", 2**64), ("to", bytes(31)), ("from_", bytes(33)),
                         ("signer_pubkey", b"")):
        t = T.SignedTransfer(**vars(g))
        setattr(t, field, value)
        with pytest.raises(ValueError):
            T.pack([g, t])


def test_dispatch_follows_the_verifier_and_the_keyword():
    class Recording(T.ModelVerifier):
        """auth_records by the model over the packed fields: what the device computes"""
        calls = 0

        def auth_records(self, rec):
            Recording.calls += 1
            items = []
            for r in rec:
                f = (r["from"].tobytes(), r["to"].tobytes(), int(r["amount"]), int(r["nonce"]))
                cls, extra = (T.SignedWithdrawal, ()) if r["kind"] else (T.SignedTransfer, (int(r["chain_id"]),))
                items.append(cls(*f, *extra, r["signature"].tobytes(), r["signer_pubkey"].tobytes()))
            reasons, formats = T._verify(T.ModelVerifier(), items)
            return (np.array([T._REASONS.index(x) for x in reasons], np.uint8),
                    np.array([T._FORMATS.index(x) for x in formats], np.uint8))

    g = T.sign_transfer(SEED, bytes(32), 1, 2, 3, legacy=True)
    bad = T.SignedTransfer(g.from_, g.to, 2, 2, 3, g.signature, g.signer_pubkey)
    short = T.SignedTransfer(g.from_, g.to, 1, 2, 3, b"\1" * 5, g.signer_pubkey)
    no_key = T.SignedTransfer(g.from_, g.to, 1, 2, 3, b"", (2).to_bytes(32, "little"))
    items = [g, bad, short, no_key, T.sign_withdrawal(SEED, b"\xff" * 32, 7, 8)]
    want = ([T.OK, T.VERIFICATION_FAILED, T.INVALID_SIGNATURE_LENGTH, T.INVALID_PUBKEY, T.OK],
            [T.LEGACY, None, None, None, T.READABLE])
    assert T.verify_signed(T.ModelVerifier(), items) == want
    assert T.verify_signed(Recording(), items) == want and Recording.calls == 1
    assert T.verify_signed(Recording(), items, device_messages=True) == want and Recording.calls == 2
    assert T.verify_signed(Recording(), items, device_messages=False) == want and Recording.calls == 2
    with pytest.raises(ValueError):
        T.verify_signed(T.ModelVerifier(), items, device_messages=True)
