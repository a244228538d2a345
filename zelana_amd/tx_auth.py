"""Authorisation of the transparent path's transactions: the Ed25519 checks the
reference's sequencer makes before it touches an account
(core/src/sequencer/execution/tx_router.rs:668-793, verify_transfer_signature
and verify_withdraw_signature), over gpu.Ed25519Verifier.

verify_transfers / verify_withdrawals give one reason per transaction, in the
order of the reference's `bail!`s:
  INVALID_PUBKEY             signer_pubkey does not decompress (VerifyingKey::from_bytes)
  INVALID_SIGNATURE_LENGTH   the signature is not 64 bytes
  VERIFICATION_FAILED        neither message format verifies (s >= L included)
  FROM_MISMATCH              a format verified, and `from` is not signer_pubkey
  OK
The human-readable message is tried first, for all transactions in one
verify_many; the legacy binary message is tried in a second verify_many over
the failures alone.  The messages are built in Python (ed25519.py); building
them on the device is not part of this."""
from __future__ import annotations

from dataclasses import dataclass

from . import ed25519 as E
from .r1cs import R

OK = "ok"
INVALID_PUBKEY = "invalid signer public key"
INVALID_SIGNATURE_LENGTH = "invalid signature length"
VERIFICATION_FAILED = "signature verification failed"
FROM_MISMATCH = "from address mismatch"
READABLE, LEGACY = "readable", "legacy"


@dataclass
class SignedTransfer:
    """The reference's SignedTransaction (sdk/transaction/src/lib.rs:68-85):
    data.{from, to, amount, nonce, chain_id}, signature, signer_pubkey"""
    from_: bytes
    to: bytes
    amount: int
    nonce: int
    chain_id: int
    signature: bytes
    signer_pubkey: bytes

    def messages(self):
        f = (self.from_, self.to, self.amount, self.nonce, self.chain_id)
        return E.transfer_message(*f), E.legacy_transfer_message(*f)


@dataclass
class SignedWithdrawal:
    """The reference's WithdrawRequest (core/src/api/types.rs:190-203)"""
    from_: bytes
    to_l1_address: bytes
    amount: int
    nonce: int
    signature: bytes
    signer_pubkey: bytes

    def messages(self):
        f = (self.from_, self.to_l1_address, self.amount, self.nonce)
        return E.withdraw_message(*f), E.legacy_withdraw_message(*f)


def sign_transfer(seed: bytes, to: bytes, amount: int, nonce: int, chain_id: int, legacy: bool = False) -> SignedTransfer:
    """a transfer from the seed's own key, signed by the model (tests and tools)"""
    pk = E.public_key(seed)
    t = SignedTransfer(pk, bytes(to), amount, nonce, chain_id, b"", pk)
    t.signature = E.sign(seed, t.messages()[1 if legacy else 0])
    return t


def sign_withdrawal(seed: bytes, to_l1: bytes, amount: int, nonce: int, legacy: bool = False) -> SignedWithdrawal:
    pk = E.public_key(seed)
    w = SignedWithdrawal(pk, bytes(to_l1), amount, nonce, b"", pk)
    w.signature = E.sign(seed, w.messages()[1 if legacy else 0])
    return w


def signature_field(signature: bytes) -> int:
    """what the batch circuit's `signature` input carries: the first 31 bytes
    of the signature as a big-endian integer (the reference hands the circuit
    the signature's hex).  The circuit does not constrain it."""
    return int.from_bytes(bytes(signature)[:31], "big")


def _verify(verifier, items):
    """-> ([reason], [format or None])"""
    items = list(items)
    n = len(items)
    if n == 0:
        return [], []
    if any(len(bytes(t.signer_pubkey)) != 32 or len(bytes(t.from_)) != 32 for t in items):
        raise ValueError("32-byte signer_pubkey and from")
    msgs = [t.messages() for t in items]
    # a signature of the wrong length goes in as zeros: the key is judged first
    sigs = [bytes(t.signature) if len(bytes(t.signature)) == 64 else bytes(64) for t in items]
    pks = [bytes(t.signer_pubkey) for t in items]
    v = verifier.verify_many(pks, [m[0] for m in msgs], sigs)
    reasons, formats, retry = [None] * n, [None] * n, []
    for i, t in enumerate(items):
        if v[i] == E.SIG_BAD_PUBKEY:
            reasons[i] = INVALID_PUBKEY
        elif len(bytes(t.signature)) != 64:
            reasons[i] = INVALID_SIGNATURE_LENGTH
        elif v[i] == E.SIG_OK:
            formats[i] = READABLE
        else:
            retry.append(i)
    if retry:
        v2 = verifier.verify_many([pks[i] for i in retry], [msgs[i][1] for i in retry], [sigs[i] for i in retry])
        for i, r in zip(retry, v2):
            if r == E.SIG_OK:
                formats[i] = LEGACY
            else:
                reasons[i] = VERIFICATION_FAILED
    for i, t in enumerate(items):
        if formats[i] is not None:
            reasons[i] = OK if bytes(t.from_) == bytes(t.signer_pubkey) else FROM_MISMATCH
    return reasons, formats


def verify_signed(verifier, items):
    """transfers and withdrawals mixed, in one pass -> ([reason], [format])"""
    return _verify(verifier, items)


def verify_transfers(verifier, txs):
    """txs: SignedTransfer each -> ([reason], [READABLE / LEGACY / None]);
    verifier: anything with verify_many(pubkeys, msgs, sigs) -> SIG_* codes"""
    return _verify(verifier, txs)


def verify_withdrawals(verifier, reqs):
    """reqs: SignedWithdrawal each -> ([reason], [READABLE / LEGACY / None])"""
    return _verify(verifier, reqs)


class ModelVerifier:
    """verify_many by the plain-Python model: the oracle of the tests"""

    def verify_many(self, pubkeys, msgs, sigs):
        return [E.verify(p, m, s) for p, m, s in zip(pubkeys, msgs, sigs)]


def transfer_tuple(t: SignedTransfer):
    """the (sender id, receiver id, amount, signature) DeviceAccountState.batches takes"""
    return bytes(t.from_), bytes(t.to), int(t.amount), signature_field(t.signature)


def withdrawal_tuple(w: SignedWithdrawal):
    """(sender id, l1_recipient, amount, signature); the recipient as the
    big-endian integer of its 32 bytes mod r"""
    return bytes(w.from_), int.from_bytes(bytes(w.to_l1_address), "big") % R, int(w.amount), signature_field(w.signature)
