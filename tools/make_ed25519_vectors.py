#!/usr/bin/env python3
"""Write tests/golden/ed25519_vectors.json from OpenSSL 3's libcrypto (through
ctypes): Ed25519 public keys, signatures and verification verdicts that do not
come from this project's own code.  The tests read only the JSON.

    python tools/make_ed25519_vectors.py [--out PATH]

Inputs are drawn from a fixed seed, so a rerun on any machine with OpenSSL 3
rewrites the same file.  Two sections:
  "sign":   seed -> (public key, signature) from EVP_DigestSign, for the
            message lengths at which 64 + len crosses SHA-512's block and
            padding boundaries;
  "verify": crafted (public key, message, signature) triples with the verdict
            of EVP_DigestVerify ("ok") and the reason the construction implies
            ("reason", a ZKMI_SIG_* code).
The small integer model below only builds the crafted cases (small-order and
non-canonical points, chosen scalars); every recorded verdict is libcrypto's.
"""
from __future__ import annotations

import argparse
import ctypes
import ctypes.util
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVP_PKEY_ED25519 = 1087
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SIGN_LENS = [0, 1, 47, 48, 63, 64, 65, 175, 176, 300]
OK, BAD_PUBKEY, BAD_S, MISMATCH = 0, 1, 2, 3


# ------------------------------------------------------------------ libcrypto
def load_libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        raise SystemExit("no libcrypto on this machine")
    C = ctypes.CDLL(name)
    vp, cp, ip, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t
    C.EVP_PKEY_new_raw_private_key.restype = vp
    C.EVP_PKEY_new_raw_private_key.argtypes = [ip, vp, cp, sz]
    C.EVP_PKEY_new_raw_public_key.restype = vp
    C.EVP_PKEY_new_raw_public_key.argtypes = [ip, vp, cp, sz]
    C.EVP_PKEY_get_raw_public_key.argtypes = [vp, cp, ctypes.POINTER(sz)]
    C.EVP_PKEY_free.argtypes = [vp]
    C.EVP_MD_CTX_new.restype = vp
    C.EVP_MD_CTX_free.argtypes = [vp]
    C.EVP_DigestSignInit.argtypes = [vp, vp, vp, vp, vp]
    C.EVP_DigestSign.argtypes = [vp, cp, ctypes.POINTER(sz), cp, sz]
    C.EVP_DigestVerifyInit.argtypes = [vp, vp, vp, vp, vp]
    C.EVP_DigestVerify.argtypes = [vp, cp, sz, cp, sz]
    C.ERR_clear_error.restype = None
    return C


def ossl_keypair_sign(C, seed: bytes, msg: bytes):
    """-> (public key, signature)"""
    sk = C.EVP_PKEY_new_raw_private_key(EVP_PKEY_ED25519, None, seed, 32)
    assert sk
    pk = ctypes.create_string_buffer(32)
    n = ctypes.c_size_t(32)
    assert C.EVP_PKEY_get_raw_public_key(sk, pk, ctypes.byref(n)) == 1 and n.value == 32
    md = C.EVP_MD_CTX_new()
    assert C.EVP_DigestSignInit(md, None, None, None, sk) == 1
    sig = ctypes.create_string_buffer(64)
    n = ctypes.c_size_t(64)
    assert C.EVP_DigestSign(md, sig, ctypes.byref(n), msg, len(msg)) == 1 and n.value == 64
    C.EVP_MD_CTX_free(md)
    C.EVP_PKEY_free(sk)
    return pk.raw, sig.raw


def ossl_verify(C, pk: bytes, msg: bytes, sig: bytes) -> bool:
    key = C.EVP_PKEY_new_raw_public_key(EVP_PKEY_ED25519, None, pk, 32)
    assert key  # the raw key is only stored here; it is decoded by the verification
    md = C.EVP_MD_CTX_new()
    assert C.EVP_DigestVerifyInit(md, None, None, None, key) == 1
    ok = C.EVP_DigestVerify(md, sig, len(sig), msg, len(msg)) == 1
    C.ERR_clear_error()
    C.EVP_MD_CTX_free(md)
    C.EVP_PKEY_free(key)
    return ok


# ------------------------------------------ the integer model of the crafting
def add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def mul(k, p):
    q = (0, 1)
    while k:
        if k & 1:
            q = add(q, p)
        p = add(p, p)
        k >>= 1
    return q


def enc(p) -> bytes:
    return (p[1] | (p[0] & 1) << 255).to_bytes(32, "little")


def x_of(y: int, sign: int):
    """an x for y (any parity when x = 0), or None when y is on no point"""
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x2 = u * pow(v, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    if (x * x - x2) % P:
        return None
    return P - x if x & 1 != sign and x else x


BASE = (x_of(4 * pow(5, P - 2, P) % P, 0), 4 * pow(5, P - 2, P) % P)
le32 = lambda v: v.to_bytes(32, "little")


def challenge(r: bytes, a: bytes, m: bytes) -> int:
    return int.from_bytes(hashlib.sha512(r + a + m).digest(), "little") % L


def stream(seed: str):
    i = 0
    while True:
        yield hashlib.sha256(f"{seed}/{i}".encode()).digest()
        i += 1


def order8_point(rnd):
    while True:
        y = int.from_bytes(next(rnd), "little") % P
        x = x_of(y, 0)
        if x is None:
            continue
        t = mul(L, (x, y))  # the torsion part
        if mul(4, t) != (0, 1):
            return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ed25519_vectors.json"))
    args = ap.parse_args()
    C = load_libcrypto()
    rnd = stream("zelana-ed25519-vectors")
    signs = []
    for n in SIGN_LENS:
        seed = next(rnd)
        msg = b"".join(next(rnd) for _ in range(10))[:n]
        pk, sig = ossl_keypair_sign(C, seed, msg)
        signs.append({"len": n, "seed": seed.hex(), "msg": msg.hex(), "public_key": pk.hex(), "signature": sig.hex()})

    cases = []

    def case(name, pk, msg, sig, reason):
        cases.append({"name": name, "public_key": pk.hex(), "msg": msg.hex(), "signature": sig.hex(),
                      "ok": ossl_verify(C, pk, msg, sig), "reason": reason})

    seed, msg = next(rnd), b"a transfer of 5 lamports, or so this message says"
    pk, sig = ossl_keypair_sign(C, seed, msg)
    flip = lambda b, bit: bytes(x ^ (1 << (bit % 8)) if i == bit // 8 else x for i, x in enumerate(b))
    case("honest", pk, msg, sig, OK)
    case("changed message", pk, msg + b"!", sig, MISMATCH)
    case("one bit of R flipped", pk, msg, flip(sig, 13), MISMATCH)
    case("one bit of s flipped", pk, msg, flip(sig, 256 + 13), MISMATCH)
    # the first flipped bit of A that still decompresses, and the first that does not
    on_curve = lambda a: x_of((int.from_bytes(a, "little") & (2**255 - 1)) % P, 0) is not None
    bit_on = next(b for b in range(13, 255) if on_curve(flip(pk, b)))
    bit_off = next(b for b in range(13, 255) if not on_curve(flip(pk, b)))
    case("one bit of A flipped, still a point", flip(pk, bit_on), msg, sig, MISMATCH)
    case("one bit of A flipped, no point", flip(pk, bit_off), msg, sig, BAD_PUBKEY)
    s = int.from_bytes(sig[32:], "little")
    case("s + L", pk, msg, sig[:32] + le32(s + L), BAD_S)

    r7 = enc(mul(7, BASE))
    for name, a in (("A = identity, (R, s) = ([7]B, 7)", le32(1)),
                    ("A = identity encoded as y = p + 1", le32(P + 1)),
                    ("A = identity with the sign bit set on x = 0", le32(1 | 1 << 255))):
        case(name, a, b"small order", r7 + le32(7), OK)

    t8 = enc(order8_point(rnd))
    r = 1 + int.from_bytes(next(rnd), "little") % (L - 1)
    rb = enc(mul(r, BASE))
    want = {True: None, False: None}
    i = 0
    while None in want.values():
        m = f"order-8 public key, message {i}".encode()
        hit = challenge(rb, t8, m) % 8 == 0
        if want[hit] is None:
            want[hit] = m
        i += 1
    case("A of order 8, k = 0 mod 8", t8, want[True], rb + le32(r), OK)
    case("A of order 8, k != 0 mod 8", t8, want[False], rb + le32(r), MISMATCH)

    case("s = 0, A = identity, R = identity", le32(1), b"nothing", le32(1) + le32(0), OK)
    case("s = 0, A = identity, R = identity encoded as p + 1", le32(1), b"nothing", le32(P + 1) + le32(0), MISMATCH)

    y = 2
    while x_of(y, 0) is not None:
        y += 1
    case("A not on the curve", le32(y), msg, sig, BAD_PUBKEY)
    case("s = L - 1", pk, msg, sig[:32] + le32(L - 1), MISMATCH)
    case("s = L", pk, msg, sig[:32] + le32(L), BAD_S)
    for c in cases:
        assert c["ok"] == (c["reason"] == OK), ("libcrypto disagrees with the construction", c["name"])

    with open(args.out, "w") as f:
        json.dump({"source": "OpenSSL 3 libcrypto: EVP_DigestSign / EVP_DigestVerify (ED25519)",
                   "sign": signs, "verify": cases}, f, indent=1)
        f.write("\n")
    print("wrote", args.out, len(signs), "signing and", len(cases), "verification cases")


if __name__ == "__main__":
    main()
