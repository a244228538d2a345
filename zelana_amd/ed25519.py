"""Ed25519 in plain Python: the model the device code (csrc/ed25519.h) is held
to, the signer of the tests, and the builder of the messages the sequencer's
transparent path signs.

verify() follows ed25519-dalek 2.2.0 `Verifier::verify` (not verify_strict),
which is what the reference calls in
core/src/sequencer/execution/tx_router.rs:668-793:
  * the public key is decompressed by curve25519-dalek 4.1.3's rules: bit 255
    is the sign of x, the low 255 bits are y and need not be below p (they are
    reduced), x = 0 with the sign bit set is accepted; only a y for which
    (y^2 - 1) / (d y^2 + 1) is no square fails                -> SIG_BAD_PUBKEY
  * s >= L is refused                                          -> SIG_BAD_S
  * k = SHA-512(R || A as given || M) mod L, R' = [s]B + [k](-A), and the
    canonical 32 bytes of R' are compared with the signature's R.  No cofactor
    is multiplied in, a small-order A is accepted, and a non-canonical R fails
    because its bytes differ, not because it was decoded       -> SIG_MISMATCH
  * otherwise                                                  -> SIG_OK
A public key that fails is reported before an s that fails: the reference
parses the key first.

Nothing here is constant time; the signer is for tests and tools only."""
from __future__ import annotations

import hashlib
import struct

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
SIG_OK, SIG_BAD_PUBKEY, SIG_BAD_S, SIG_MISMATCH = 0, 1, 2, 3  # ZKMI_SIG_*

IDENTITY = (0, 1, 1, 0)  # extended coordinates (X, Y, Z, T), x = X / Z, y = Y / Z, T = X Y / Z


def point_add(p, q):
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


def point_neg(p):
    return (-p[0] % P, p[1], p[2], -p[3] % P)


def point_mul(k: int, p):
    q = IDENTITY
    while k:
        if k & 1:
            q = point_add(q, p)
        p = point_add(p, p)
        k >>= 1
    return q


def point_eq(p, q) -> bool:
    return (p[0] * q[2] - q[0] * p[2]) % P == 0 and (p[1] * q[2] - q[1] * p[2]) % P == 0


def affine(p):
    zi = pow(p[2], P - 2, P)
    return p[0] * zi % P, p[1] * zi % P


def compress(p) -> bytes:
    x, y = affine(p)
    return (y | (x & 1) << 255).to_bytes(32, "little")


def decompress(b: bytes):
    """curve25519-dalek 4.1.3 CompressedEdwardsY::decompress -> a point or None"""
    b = bytes(b)
    if len(b) != 32:
        return None
    v = int.from_bytes(b, "little")
    sign, y = v >> 255, (v & (2**255 - 1)) % P
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    # x = sqrt(u / w): the candidate (u / w)^((p + 3) / 8), fixed up by sqrt(-1)
    x = u * pow(w, 3, P) * pow(u * pow(w, 7, P), (P - 5) // 8, P) % P
    c = w * x * x % P
    if c == (-u) % P:
        x = x * SQRT_M1 % P
    elif c != u:
        return None
    if x & 1 != sign:
        x = -x % P  # x = 0 stays 0: the sign bit of a zero x is not checked
    return (x, y, 1, x * y % P)


BASE = decompress((4 * pow(5, P - 2, P) % P).to_bytes(32, "little"))


def sc_reduce(b: bytes) -> int:
    return int.from_bytes(b, "little") % L


def _expand(seed: bytes):
    h = hashlib.sha512(bytes(seed)).digest()
    a = int.from_bytes(h[:32], "little")
    a = (a & ((1 << 254) - 8)) | 1 << 254
    return a, h[32:]


def public_key(seed: bytes) -> bytes:
    """RFC 8032 section 5.1.5"""
    assert len(seed) == 32
    return compress(point_mul(_expand(seed)[0], BASE))


def sign(seed: bytes, msg: bytes) -> bytes:
    """RFC 8032 section 5.1.6: deterministic, 64 bytes R || s"""
    a, prefix = _expand(seed)
    pk = compress(point_mul(a, BASE))
    r = sc_reduce(hashlib.sha512(prefix + bytes(msg)).digest())
    rb = compress(point_mul(r, BASE))
    k = sc_reduce(hashlib.sha512(rb + pk + bytes(msg)).digest())
    return rb + ((r + k * a) % L).to_bytes(32, "little")


def challenge(r: bytes, pk: bytes, msg: bytes) -> int:
    """k = SHA-512(R || A || M) mod L over the bytes as given"""
    return sc_reduce(hashlib.sha512(bytes(r) + bytes(pk) + bytes(msg)).digest())


def verify_core(r: bytes, a_point, k: int, s: int) -> bool:
    """compress([s]B + [k](-A)) == R, bytewise (dalek's recompute_R)"""
    rp = point_add(point_mul(s, BASE), point_mul(k, point_neg(a_point)))
    return compress(rp) == bytes(r)


def verify(pk: bytes, msg: bytes, sig: bytes) -> int:
    """-> SIG_OK / SIG_BAD_PUBKEY / SIG_BAD_S / SIG_MISMATCH"""
    pk, sig = bytes(pk), bytes(sig)
    if len(pk) != 32 or len(sig) != 64:
        raise ValueError("verify: a 32-byte public key and a 64-byte signature")
    a = decompress(pk)
    if a is None:
        return SIG_BAD_PUBKEY
    s = int.from_bytes(sig[32:], "little")
    if s >= L:
        return SIG_BAD_S
    return SIG_OK if verify_core(sig[:32], a, challenge(sig[:32], pk, msg), s) else SIG_MISMATCH


# ---------------------------------------------------------------- the messages
_B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"  # the Bitcoin alphabet (bs58's default)
U64 = 2**64


def base58(b: bytes) -> str:
    b = bytes(b)
    v, out = int.from_bytes(b, "big"), ""
    while v:
        v, r = divmod(v, 58)
        out = _B58[r] + out
    return "1" * (len(b) - len(b.lstrip(b"\0"))) + out


def _fields(*ids, ints):
    if any(len(bytes(i)) != 32 for i in ids) or any(not 0 <= int(v) < U64 for v in ints):
        raise ValueError("32-byte ids and u64 integers")


def transfer_message(frm: bytes, to: bytes, amount: int, nonce: int, chain_id: int) -> bytes:
    """tx_router.rs:624-645 build_transfer_message, byte for byte"""
    _fields(frm, to, ints=(amount, nonce, chain_id))
    return (f"Zelana L2 Transfer\n\nFrom: {bytes(frm).hex()}\nTo: {bytes(to).hex()}\nAmount: {int(amount)} lamports\n"
            f"Nonce: {int(nonce)}\nChain ID: {int(chain_id)}\n\nSign to authorize this L2 transfer.").encode()


def withdraw_message(frm: bytes, to_l1: bytes, amount: int, nonce: int) -> bytes:
    """tx_router.rs:647-666 build_withdraw_message: `from` in lower-case hex,
    the L1 address in base58"""
    _fields(frm, to_l1, ints=(amount, nonce))
    return (f"Zelana L2 Withdrawal\n\nFrom: {bytes(frm).hex()}\nTo L1: {base58(to_l1)}\nAmount: {int(amount)} lamports\n"
            f"Nonce: {int(nonce)}\n\nSign to authorize this withdrawal to Solana L1.").encode()


def legacy_transfer_message(frm: bytes, to: bytes, amount: int, nonce: int, chain_id: int) -> bytes:
    """The reference's fallback, wincode::serialize(&tx.data).  ASSUMPTION: the
    wincode crate's source was not at hand; its layout of TransactionData is
    taken to be the fields in declaration order, ids raw and integers as
    fixed-width little-endian u64: from || to || amount || nonce || chain_id,
    88 bytes."""
    _fields(frm, to, ints=(amount, nonce, chain_id))
    return bytes(frm) + bytes(to) + struct.pack("<QQQ", int(amount), int(nonce), int(chain_id))


def legacy_withdraw_message(frm: bytes, to_l1: bytes, amount: int, nonce: int) -> bytes:
    """tx_router.rs:774-779: from || to_l1 || amount le64 || nonce le64, 80 bytes"""
    _fields(frm, to_l1, ints=(amount, nonce))
    return bytes(frm) + bytes(to_l1) + struct.pack("<QQ", int(amount), int(nonce))
