"""CPU: the plain-Python model of note encryption (zelana_amd/note_crypt.py)
against answers that are not its own: X25519 and ChaCha20-Poly1305 from
OpenSSL's libcrypto (tests/golden/note_crypt_vectors.json, written by
tools/make_note_crypt_vectors.py), the RFC 7748 / 8439 examples, and BLAKE3's
published derive_key vector for the empty input; then the note format's round
trips and refusals."""
import struct

import pytest

import note_crypt_cases as C
from zelana_amd import blake3
from zelana_amd import note_crypt as NC


def test_x25519_matches_libcrypto_and_rfc7748():
    g = C.golden()["x25519"]
    names = " ".join(c["name"] for c in g)
    for need in ("random", "u=p", "bit255", "u=0", "u=1", "u=9", "all-00", "all-FF", "2^256-1"):
        assert need in names
    for c in g:
        assert NC.x25519(bytes.fromhex(c["scalar"]), bytes.fromhex(c["u"])).hex() == c["out"], c["name"]
    assert any(c["openssl_error"] and c["out"] == "00" * 32 for c in g)
    # RFC 7748 section 5.2
    k = bytes.fromhex("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4")
    u = bytes.fromhex("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")
    assert NC.x25519(k, u).hex() == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    # section 6.1
    a = bytes.fromhex("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a")
    assert NC.public_key(a).hex() == "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"


def test_aead_matches_libcrypto():
    g = C.golden()["aead"]
    assert [c["ct_len"] for c in g] == [16, 57, 58, 63, 64, 65, 80, 122, 123, 570]
    for c in g:
        key, nonce, ct, pt = (bytes.fromhex(c[k]) for k in ("key", "nonce", "ciphertext", "plaintext"))
        assert len(ct) == c["ct_len"]
        assert NC.chacha20_poly1305_seal(key, nonce, pt) == ct
        assert NC.chacha20_poly1305_open(key, nonce, ct) == pt


def test_derive_key_reuses_the_pinned_compression():
    # blake3()'s _compress is pinned by the reference's vk-hash fixtures; derive_key adds the two mode flags
    assert blake3.DERIVE_KEY_CONTEXT == 32 and blake3.DERIVE_KEY_MATERIAL == 64
    # BLAKE3's published test vector: derive_key over the empty input
    assert blake3.derive_key("BLAKE3 2019-12-27 16:29:52 test vectors context", b"").hex() == \
        "2cc39783c223154fea8dfb7c1b1660f2ac2dcbd1c1de8277b0b0dd39b7e50d7d"
    key = NC.derive_note_key(bytes(range(32)), bytes(range(32, 64)))
    ctx = struct.unpack("<8I", NC.note_context_key())
    block = struct.unpack("<16I", bytes(range(64)))
    assert key == struct.pack("<8I", *blake3._compress(list(ctx), list(block), 0, 64, 1 | 2 | 8 | 64)[:8])
    assert NC.note_context_key() == struct.pack("<8I", *blake3._compress(
        blake3.IV, blake3._words(b"zelana-note-v1"), 0, 14, 1 | 2 | 8 | 32)[:8])


@pytest.mark.parametrize("memo_len", [0, 1, 5, 6, 22, 23, 512, 600])
def test_round_trip(memo_len):
    sk = C.rnd(f"rt/sk/{memo_len}")
    pk = NC.public_key(sk)
    rand, memo = C.rnd("rt/rand"), C.rnd("rt/memo", memo_len)
    enc = NC.encrypt_note(12345 + memo_len, rand, pk, memo or None, esk=C.rnd("rt/esk"), nonce=C.rnd("rt/n", 12))
    assert len(enc[2]) == 58 + min(memo_len, 512)
    assert enc == NC.encrypt_note(12345 + memo_len, rand, pk, memo or None, esk=C.rnd("rt/esk"), nonce=C.rnd("rt/n", 12))
    assert NC.decrypt_note(enc, sk) == (12345 + memo_len, rand, memo[:512])
    fresh = NC.encrypt_note(1, rand, pk)  # os.urandom
    assert fresh[0] != enc[0] and NC.decrypt_note(fresh, sk) == (1, rand, b"")


def test_refusals():
    sk, other = C.rnd("rf/sk"), C.rnd("rf/other")
    pk, rand = NC.public_key(sk), C.rnd("rf/rand")
    epk, nonce, ct = NC.encrypt_note(9, rand, pk, b"hello", esk=C.rnd("rf/esk"), nonce=C.rnd("rf/n", 12))
    assert NC.decrypt_note((epk, nonce, ct), sk) == (9, rand, b"hello")
    assert NC.decrypt_note((epk, nonce, ct), other) is None
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]
    assert NC.decrypt_note((flip(epk, 3), nonce, ct), sk) is None
    assert NC.decrypt_note((epk, flip(nonce, 11), ct), sk) is None
    assert NC.decrypt_note((epk, nonce, flip(ct, 0)), sk) is None
    assert NC.decrypt_note((epk, nonce, flip(ct, len(ct) - 1)), sk) is None
    assert NC.decrypt_note((epk, nonce, ct[:15]), sk) is None and NC.decrypt_note((epk, nonce, b""), sk) is None
    # a sender's own plaintexts: memo_len beyond the end, trailing bytes
    key = NC.derive_note_key(NC.x25519(sk, epk), epk)
    head = struct.pack("<Q", 9) + rand
    seal = lambda pt: (epk, nonce, NC.chacha20_poly1305_seal(key, nonce, pt))
    assert NC.decrypt_note(seal(head + struct.pack("<H", 6) + b"hello"), sk) is None
    assert NC.classify(seal(head + struct.pack("<H", 6) + b"hello"), sk, pk, bytes(32))[0] == NC.MALFORMED
    assert NC.decrypt_note(seal((head + b"\0\0")[:41]), sk) is None
    assert NC.decrypt_note(seal(head + struct.pack("<H", 2) + b"hello"), sk) == (9, rand, b"he")
    commit = lambda owner, value, r: bytes([value]) + r[1:]
    assert NC.try_decrypt_note((epk, nonce, ct), sk, pk, bytes([9]) + rand[1:], commit) == (9, rand, b"hello")
    assert NC.try_decrypt_note((epk, nonce, ct), sk, pk, bytes(32), commit) is None
    assert NC.classify((epk, nonce, ct), sk, pk, bytes(32), commit)[0] == NC.WRONG_COMMITMENT
    assert NC.classify((epk, nonce, ct), other, pk, bytes(32), commit)[0] == NC.NOT_MINE


def test_scan_model_pagination():
    sk = C.rnd("sm/sk")
    pk = NC.public_key(sk)
    notes = []
    for i, pos in enumerate([7, 3, 9, 1, 5, 8]):
        to = pk if pos != 8 else NC.public_key(C.rnd("sm/else"))
        epk, nonce, ct = NC.encrypt_note(pos, C.rnd(f"sm/r/{i}"), to, esk=C.rnd(f"sm/e/{i}"), nonce=C.rnd(f"sm/n/{i}", 12))
        notes.append((pos, bytes(32), epk, nonce, ct))
    hits, to_, stats = NC.scan_model(notes, sk, pk)
    assert [h[0] for h in hits] == [1, 3, 5, 7, 9] and to_ == 9 and stats == [1, 0, 0, 5]
    hits, to_, _ = NC.scan_model(notes, sk, pk, limit=2)
    assert [h[0] for h in hits] == [1, 3] and to_ == 3
    hits, to_, stats = NC.scan_model(notes, sk, pk, from_position=to_ + 1, limit=5)
    assert [h[0] for h in hits] == [5, 7, 9] and to_ == 9 and stats == [1, 0, 0, 3]
    assert NC.scan_model(notes, sk, pk, from_position=10) == ([], 10, [0, 0, 0, 0])
