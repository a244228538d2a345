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
The human-readable message is tried first, for all transactions, and the
legacy binary message in a second pass over the failures alone.  Two paths
give the same answer:
  * the device path (a verifier with auth_records, which gpu.Ed25519Verifier
    has): pack() turns the transactions into fixed-width records, and the
    device builds both messages, verifies, retries and compares `from` with
    the signer (zkmi_tx_auth_many);
  * the host path (device_messages=False, or a verifier with verify_many
    alone, such as ModelVerifier): the messages are built in Python
    (ed25519.py) and go through two verify_many calls.
A signature of the wrong length is a host matter on both."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

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


def pack(items):
    """SignedTransfer / SignedWithdrawal each -> the records auth_records takes
    (gpu.SIGNED_TX_DTYPE, the C ABI's zkmi_signed_tx).  No message is built
    here.  A signature that is not 64 bytes goes in as zeros."""
    from .gpu import SIGNED_TX_DTYPE, TX_TRANSFER, TX_WITHDRAWAL
    items = list(items)
    n = len(items)
    kinds = [TX_WITHDRAWAL if isinstance(t, SignedWithdrawal) else TX_TRANSFER for t in items]
    tos = [t.to_l1_address if k else t.to for t, k in zip(items, kinds)]
    if any(len(t.from_) != 32 or len(t.signer_pubkey) != 32 or len(to) != 32 for t, to in zip(items, tos)):
        raise ValueError("32-byte from, to and signer_pubkey")
    blob = b"".join([b"".join((t.from_, to, t.signer_pubkey, t.signature if len(t.signature) == 64 else bytes(64)))
                     for t, to in zip(items, tos)])
    rec = np.zeros(n, SIGNED_TX_DTYPE)
    cols = np.frombuffer(blob, np.uint8).reshape(n, 160)
    rec["from"], rec["to"], rec["signer_pubkey"], rec["signature"] = cols[:, :32], cols[:, 32:64], cols[:, 64:96], cols[:, 96:]
    ints = {"amount": [int(t.amount) for t in items], "nonce": [int(t.nonce) for t in items],
            "chain_id": [0 if k else int(t.chain_id) for t, k in zip(items, kinds)]}
    for name, column in ints.items():
        if n and not (0 <= min(column) and max(column) < E.U64):
            raise ValueError("u64 amount, nonce and chain_id")
        rec[name] = np.array(column, np.uint64)
    rec["kind"] = kinds
    return rec


_REASONS = (OK, INVALID_PUBKEY, VERIFICATION_FAILED, FROM_MISMATCH)  # gpu.TXAUTH_*
_FORMATS = (None, READABLE, LEGACY)                                   # gpu.TXFMT_*


def _verify_on_device(verifier, items):
    r, f = verifier.auth_records(pack(items))
    reasons, formats = [_REASONS[v] for v in r.tolist()], [_FORMATS[v] for v in f.tolist()]
    for i in [i for i, t in enumerate(items) if len(t.signature) != 64]:
        if reasons[i] != INVALID_PUBKEY:
            reasons[i], formats[i] = INVALID_SIGNATURE_LENGTH, None
    return reasons, formats


def _verify(verifier, items, device_messages=None):
    """-> ([reason], [format or None]).  device_messages: None takes the device
    path when the verifier has auth_records, False the host path, True the
    device path or a ValueError."""
    items = list(items)
    n = len(items)
    if n == 0:
        return [], []
    if device_messages is None:
        device_messages = hasattr(verifier, "auth_records")
    if device_messages:
        if not hasattr(verifier, "auth_records"):
            raise ValueError("device_messages=True needs a verifier with auth_records")
        return _verify_on_device(verifier, items)  # pack() checks the lengths
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


def verify_signed(verifier, items, device_messages: bool | None = None):
    """transfers and withdrawals mixed, in one pass -> ([reason], [format])"""
    return _verify(verifier, items, device_messages)


def verify_transfers(verifier, txs, device_messages: bool | None = None):
    """txs: SignedTransfer each -> ([reason], [READABLE / LEGACY / None]);
    verifier: anything with verify_many(pubkeys, msgs, sigs) -> SIG_* codes,
    or with auth_records as well (gpu.Ed25519Verifier).  device_messages: None
    builds the messages on the device when the verifier has auth_records,
    False builds them in Python; the result is the same."""
    return _verify(verifier, txs, device_messages)


def verify_withdrawals(verifier, reqs, device_messages: bool | None = None):
    """reqs: SignedWithdrawal each -> ([reason], [READABLE / LEGACY / None])"""
    return _verify(verifier, reqs, device_messages)


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
