#!/usr/bin/env python3
"""Write tests/golden/note_crypt_vectors.json from OpenSSL 3's libcrypto
(through ctypes): X25519 and ChaCha20-Poly1305 answers that do not come from
this project's own code.  The tests read only the JSON.

    python tools/make_note_crypt_vectors.py [--out PATH]

Inputs are drawn from a fixed seed, so a rerun on any machine with OpenSSL 3
rewrites the same file.  For a low-order u OpenSSL's EVP_PKEY_derive reports
an error; the bytes it would have returned are all zero (x25519-dalek's
diffie_hellman, which the reference calls, returns them and carries on), and
that is what is recorded, with "openssl_error": true beside it.
"""
from __future__ import annotations

import argparse
import ctypes
import ctypes.util
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVP_PKEY_X25519 = 1034
CTRL_AEAD_SET_IVLEN, CTRL_AEAD_GET_TAG, CTRL_AEAD_SET_TAG = 0x9, 0x10, 0x11
P = 2**255 - 19
# the AEAD body lengths behind the scan test's ciphertext lengths (tag excluded)
CT_LENS = [16, 57, 58, 63, 64, 65, 80, 122, 123, 570]


def load_libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        raise SystemExit("no libcrypto on this machine")
    L = ctypes.CDLL(name)
    vp, cp, ip, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t
    L.EVP_PKEY_new_raw_private_key.restype = vp
    L.EVP_PKEY_new_raw_private_key.argtypes = [ip, vp, cp, sz]
    L.EVP_PKEY_new_raw_public_key.restype = vp
    L.EVP_PKEY_new_raw_public_key.argtypes = [ip, vp, cp, sz]
    L.EVP_PKEY_CTX_new.restype = vp
    L.EVP_PKEY_CTX_new.argtypes = [vp, vp]
    L.EVP_PKEY_derive_init.argtypes = [vp]
    L.EVP_PKEY_derive_set_peer.argtypes = [vp, vp]
    L.EVP_PKEY_derive.argtypes = [vp, cp, ctypes.POINTER(sz)]
    L.EVP_PKEY_CTX_free.argtypes = [vp]
    L.EVP_PKEY_free.argtypes = [vp]
    L.EVP_chacha20_poly1305.restype = vp
    L.EVP_CIPHER_CTX_new.restype = vp
    L.EVP_CIPHER_CTX_free.argtypes = [vp]
    L.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, cp, cp]
    L.EVP_EncryptUpdate.argtypes = [vp, cp, ctypes.POINTER(ip), cp, ip]
    L.EVP_EncryptFinal_ex.argtypes = [vp, cp, ctypes.POINTER(ip)]
    L.EVP_CIPHER_CTX_ctrl.argtypes = [vp, ip, ip, vp]
    return L


def ossl_x25519(L, scalar: bytes, u: bytes):
    """-> (32 bytes, openssl reported an error)"""
    sk = L.EVP_PKEY_new_raw_private_key(EVP_PKEY_X25519, None, scalar, 32)
    pk = L.EVP_PKEY_new_raw_public_key(EVP_PKEY_X25519, None, u, 32)
    ctx = L.EVP_PKEY_CTX_new(sk, None)
    assert sk and pk and ctx
    assert L.EVP_PKEY_derive_init(ctx) == 1 and L.EVP_PKEY_derive_set_peer(ctx, pk) == 1
    out = ctypes.create_string_buffer(32)
    n = ctypes.c_size_t(32)
    ok = L.EVP_PKEY_derive(ctx, out, ctypes.byref(n)) == 1
    L.EVP_PKEY_CTX_free(ctx)
    L.EVP_PKEY_free(sk)
    L.EVP_PKEY_free(pk)
    return (out.raw if ok else bytes(32)), not ok


def ossl_seal(L, key: bytes, nonce: bytes, pt: bytes) -> bytes:
    ctx = L.EVP_CIPHER_CTX_new()
    assert L.EVP_EncryptInit_ex(ctx, L.EVP_chacha20_poly1305(), None, None, None) == 1
    assert L.EVP_CIPHER_CTX_ctrl(ctx, CTRL_AEAD_SET_IVLEN, 12, None) == 1
    assert L.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
    out = ctypes.create_string_buffer(len(pt) + 16)
    n = ctypes.c_int(0)
    if pt:
        assert L.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
    tail = ctypes.create_string_buffer(16)
    m = ctypes.c_int(0)
    assert L.EVP_EncryptFinal_ex(ctx, tail, ctypes.byref(m)) == 1
    tag = ctypes.create_string_buffer(16)
    assert L.EVP_CIPHER_CTX_ctrl(ctx, CTRL_AEAD_GET_TAG, 16, tag) == 1
    L.EVP_CIPHER_CTX_free(ctx)
    return out.raw[:n.value] + tag.raw


def stream(seed: str):
    i = 0
    while True:
        yield hashlib.sha256(f"{seed}/{i}".encode()).digest()
        i += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "note_crypt_vectors.json"))
    args = ap.parse_args()
    L = load_libcrypto()
    rnd = stream("zelana-note-crypt-vectors")
    le = lambda v: v.to_bytes(32, "little")
    xs = []
    for name, scalar, u in (
            [(f"random{i}", next(rnd), next(rnd)) for i in range(6)] +
            [("u=p", next(rnd), le(P)), ("u=p+1", next(rnd), le(P + 1)), ("u=2^255-1", next(rnd), le(2**255 - 1)),
             ("u=p-1", next(rnd), le(P - 1)),
             ("bit255 set", next(rnd), le(9 | 1 << 255)), ("bit255 set random", next(rnd), le(int.from_bytes(next(rnd), "little") | 1 << 255)),
             ("u=2^256-1", next(rnd), le(2**256 - 1)),
             ("u=0", next(rnd), le(0)), ("u=1", next(rnd), le(1)), ("u=9", next(rnd), le(9)),
             ("scalar all-00", bytes(32), next(rnd)), ("scalar all-FF", b"\xff" * 32, next(rnd)),
             ("scalar all-00, u=9", bytes(32), le(9)), ("scalar all-FF, u=9", b"\xff" * 32, le(9))]):
        out, err = ossl_x25519(L, scalar, u)
        xs.append({"name": name, "scalar": scalar.hex(), "u": u.hex(), "out": out.hex(), "openssl_error": err})
    aead = []
    for ct_len in CT_LENS:
        key, nonce = next(rnd), next(rnd)[:12]
        pt = b"".join(next(rnd) for _ in range(19))[:ct_len - 16]
        aead.append({"ct_len": ct_len, "key": key.hex(), "nonce": nonce.hex(), "plaintext": pt.hex(),
                     "ciphertext": ossl_seal(L, key, nonce, pt).hex()})
    with open(args.out, "w") as f:
        json.dump({"source": "OpenSSL 3 libcrypto: EVP_PKEY_derive (X25519), EVP_chacha20_poly1305 (empty AAD)",
                   "x25519": xs, "aead": aead}, f, indent=1)
        f.write("\n")
    print("wrote", args.out, len(xs), "x25519 and", len(aead), "aead cases")


if __name__ == "__main__":
    main()
