"""Cases for the op table of tests/device/note_crypt_ops.h, shared by the host
check (test_note_crypt_cpu.py) and the device probe (test_gpu_note_scan.py).
A case is (name, op, input words, check); check(output words) asserts against
Python integers mod p, the golden vectors, or the model
(zelana_amd/note_crypt.py).  The bounds are note_crypt.h's: TIGHT limbs are
below 2^26, LOOSE ones below 2^27."""
import hashlib
import json
import os
import struct

from zelana_amd import note_crypt as NC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "note_crypt_vectors.json")
P = NC.P25519
NC_IN, NC_OUT = 176, 160
(OP_FE_ADD, OP_FE_SUB, OP_FE_MUL, OP_FE_SQR, OP_FE_M121665, OP_FE_CSWAP, OP_FE_INVERT, OP_FE_LOAD, OP_FE_STORE,
 OP_X25519, OP_NOTE_KEY, OP_CHACHA, OP_POLY_MAC, OP_AEAD_PLAIN, OP_AEAD_NOTE) = range(1, 16)
TIGHT, LOOSE = 1 << 26, 1 << 27
SHIFT = [(51 * i + 1) // 2 for i in range(10)]  # ceil(25.5 i)
BITS = [26 if i % 2 == 0 else 25 for i in range(10)]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def rnd(tag: str, n: int = 32) -> bytes:
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha256(f"{tag}/{i}".encode()).digest()
        i += 1
    return out[:n]


def words(b: bytes) -> list:
    b = bytes(b) + b"\0" * (-len(b) % 4)
    return list(struct.unpack(f"<{len(b) // 4}I", b))


def unwords(w) -> bytes:
    return struct.pack(f"<{len(w)}I", *w)


def fe_val(limbs) -> int:
    return sum(int(v) << s for v, s in zip(limbs, SHIFT))


def fe_limbs(v: int) -> list:
    """the limbs fe25_load gives a value below 2^255"""
    assert 0 <= v < 1 << 255
    return [(v >> s) & ((1 << b) - 1) for s, b in zip(SHIFT, BITS)]


VALUES = [0, 1, 2, 19, P - 1, P, P + 1, 2**255 - 1, int.from_bytes(rnd("fe/a"), "little") >> 1,
          int.from_bytes(rnd("fe/b"), "little") >> 1]
LIMB_MAX = [(1 << b) - 1 for b in BITS]                   # every limb at its canonical maximum: 2^255 - 1
TIGHT_OPERANDS = [fe_limbs(v) for v in VALUES] + [LIMB_MAX, [TIGHT - 1] * 10]
LOOSE_OPERANDS = TIGHT_OPERANDS + [[LOOSE - 1] * 10]
LOAD_BYTES = [v.to_bytes(32, "little") for v in VALUES + [2**256 - 1, P + (1 << 255), 1 << 255]] + \
    [rnd(f"load/{i}") for i in range(4)]


def _check_limbs(name, out, want_value, bound):
    assert len(out) == 10, (name, len(out))
    assert all(v < bound for v in out), (name, "limb past the stated bound", [hex(v) for v in out])
    assert fe_val(out) % P == want_value % P, (name, "value")


def fe_cases():
    cs = []
    for i, a in enumerate(TIGHT_OPERANDS):
        for j, b in enumerate(TIGHT_OPERANDS):
            def chk(out, a=a, b=b, n=f"add {i} {j}"):
                _check_limbs(n, out, fe_val(a) + fe_val(b), LOOSE)
                assert list(out) == [x + y for x, y in zip(a, b)], n
            cs.append((f"fe_add {i} {j}", OP_FE_ADD, a + b, chk))
    for i, a in enumerate(LOOSE_OPERANDS):
        for j, b in enumerate(LOOSE_OPERANDS):
            cs.append((f"fe_sub {i} {j}", OP_FE_SUB, a + b,
                       lambda out, a=a, b=b, n=f"sub {i} {j}": _check_limbs(n, out, fe_val(a) - fe_val(b), TIGHT)))
            cs.append((f"fe_mul {i} {j}", OP_FE_MUL, a + b,
                       lambda out, a=a, b=b, n=f"mul {i} {j}": _check_limbs(n, out, fe_val(a) * fe_val(b), TIGHT)))
            def chk(out, a=a, b=b, bit=(i + j) & 1, n=f"cswap {i} {j}"):
                assert list(out) == ((b + a) if bit else (a + b)), n
            cs.append((f"fe_cswap {i} {j}", OP_FE_CSWAP, a + b + [(i + j) & 1], chk))
        cs.append((f"fe_sqr {i}", OP_FE_SQR, a, lambda out, a=a, n=f"sqr {i}": _check_limbs(n, out, fe_val(a) ** 2, TIGHT)))
        cs.append((f"fe_m121665 {i}", OP_FE_M121665, a,
                   lambda out, a=a, n=f"m121665 {i}": _check_limbs(n, out, fe_val(a) * 121665, TIGHT)))
        cs.append((f"fe_invert {i}", OP_FE_INVERT, a,
                   lambda out, a=a, n=f"invert {i}": _check_limbs(n, out, pow(fe_val(a) % P, P - 2, P), TIGHT)))
        def chk(out, a=a, n=f"store {i}"):
            assert unwords(out) == (fe_val(a) % P).to_bytes(32, "little"), (n, "stored bytes are not canonical")
        cs.append((f"fe_store {i}", OP_FE_STORE, a, chk))
    for i, b in enumerate(LOAD_BYTES):
        def chk(out, b=b, n=f"load {i}"):
            v = int.from_bytes(b, "little") & ((1 << 255) - 1)
            assert list(out) == fe_limbs(v), n
        cs.append((f"fe_load {i}", OP_FE_LOAD, words(b), chk))
    return cs


def x25519_cases():
    cs = []
    for c in golden()["x25519"]:
        sc, u, want = bytes.fromhex(c["scalar"]), bytes.fromhex(c["u"]), bytes.fromhex(c["out"])
        cs.append(("x25519 " + c["name"], OP_X25519, words(sc) + words(u),
                   lambda out, want=want, n=c["name"]: _eq(unwords(out), want, n)))
    # the other low-order points of RFC 7748 section 7 / the curve's twist, from the model
    for i, u in enumerate([325606250916557431795983626356110631294008115727848805560023387167927233504,
                           39382357235489614581723060781553021112529911719440698176882885853963445705823,
                           P - 1, P, P + 1]):
        sc, ub = rnd(f"x/lo/{i}"), u.to_bytes(32, "little")
        cs.append((f"x25519 low order {i}", OP_X25519, words(sc) + words(ub),
                   lambda out, want=NC.x25519(sc, ub), n=f"low {i}": _eq(unwords(out), want, n)))
    return cs


def _eq(got, want, name):
    assert got == want, (name, got.hex()[:64], want.hex()[:64])


def kdf_and_chacha_cases():
    cs = []
    ctx = NC.note_context_key()
    for i in range(4):
        ss, epk = (rnd(f"kdf/s/{i}"), rnd(f"kdf/e/{i}")) if i else (bytes(32), bytes(32))
        cs.append((f"note_key {i}", OP_NOTE_KEY, words(ctx) + words(ss) + words(epk),
                   lambda out, want=NC.derive_note_key(ss, epk), n=f"kdf {i}": _eq(unwords(out), want, n)))
    for i, ctr in enumerate([0, 1, 2, 9, 0xFFFFFFFF]):
        key, nonce = rnd(f"cc/k/{i}"), rnd(f"cc/n/{i}", 12)
        cs.append((f"chacha {i}", OP_CHACHA, words(key) + [ctr] + words(nonce),
                   lambda out, want=NC.chacha20_block(key, ctr, nonce), n=f"chacha {i}": _eq(unwords(out), want, n)))
    # RFC 8439 section 2.3.2
    key, nonce = bytes(range(32)), bytes.fromhex("000000090000004a00000000")
    want = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                         "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert NC.chacha20_block(key, 1, nonce) == want
    cs.append(("chacha rfc8439", OP_CHACHA, words(key) + [1] + words(nonce), lambda out: _eq(unwords(out), want, "rfc")))
    return cs


def poly_edge_messages():
    """[(key, msg)] whose lazy accumulator lies in [2^130 - 5, 2^130): r = 1
    with three full blocks that sum to it, r = 2 with one block that doubles
    to it; each with s = 0 and s = all-FF."""
    out = []
    le16 = lambda v: v.to_bytes(16, "little")
    for s in (bytes(16), b"\xff" * 16):
        for d in range(5):  # (2^128 + 2^127) + (2^128 + 2^127 - 5 + d) + 2^128 = 2^130 - 5 + d
            out.append((le16(1) + s, le16(1 << 127) + le16((1 << 127) - 5 + d) + le16(0)))
        for x in ((1 << 128) - 2, (1 << 128) - 1):  # 2 (2^128 + x) = 2^130 - 4, 2^130 - 2
            out.append((le16(2) + s, le16(x)))
    for key, msg in out:
        assert (1 << 130) - 5 <= NC.poly1305_lazy(key, msg) < 1 << 130
    return out


def poly_cases():
    cs = []
    msgs = list(poly_edge_messages())
    for n in (0, 1, 15, 16, 17, 64):
        msgs.append((rnd(f"poly/k/{n}"), rnd(f"poly/m/{n}", n)))
        msgs.append((rnd(f"poly/k2/{n}", 16) + b"\xff" * 16, rnd(f"poly/m2/{n}", n)))
        msgs.append((b"\xff" * 32, b"\xff" * n))
    # RFC 8439 section 2.5.2
    key = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    msg = b"Cryptographic Forum Research Group"
    assert NC.poly1305(key, msg) == bytes.fromhex("a8061dc1305136c6c22b8baf0c0127a9")
    msgs.append((key, msg))
    for i, (key, msg) in enumerate(msgs):
        cs.append((f"poly {i} len {len(msg)}", OP_POLY_MAC, words(key) + [len(msg)] + words(msg),
                   lambda out, want=NC.poly1305(key, msg), n=f"poly {i}": _eq(unwords(out), want, n)))
    return cs


def _aead_in(key, nonce, ct):
    return words(key) + words(nonce) + [len(ct)] + words(ct)


def aead_cases():
    cs = []
    for c in golden()["aead"]:
        key, nonce, ct, pt = (bytes.fromhex(c[k]) for k in ("key", "nonce", "ciphertext", "plaintext"))
        def chk(out, pt=pt, n=f"golden {c['ct_len']}"):
            assert out[0] == 1, (n, "tag refused")
            _eq(unwords(out[1:])[:len(pt)], pt, n)
            assert unwords(out[1:])[len(pt):] in (b"", b"\0", b"\0\0", b"\0\0\0"), (n, "bytes past the body are not zero")
        cs.append((f"aead golden {c['ct_len']}", OP_AEAD_PLAIN, _aead_in(key, nonce, ct), chk))
        for what, bad in (("tag", ct[:-1] + bytes([ct[-1] ^ 0x80])), ("tag0", ct[:-16] + bytes([ct[-16] ^ 1]) + ct[-15:]),
                          ("body", bytes([ct[0] ^ 1]) + ct[1:] if len(ct) > 16 else None),
                          ("short", ct[:-1]), ("long", ct + b"\0")):
            if bad is not None:
                cs.append((f"aead golden {c['ct_len']} bad {what}", OP_AEAD_PLAIN, _aead_in(key, nonce, bad),
                           lambda out, n=what: _eq(bytes(out[:1]), b"\0", n)))
    def note_chk(want, n):
        def chk(out):
            if want is None:
                assert list(out[:2]) == [1, 0], (n, "a good tag over a plaintext that does not parse", list(out[:2]))
                return
            value, rand, memo = want
            assert list(out[:2]) == [1, 1], (n, list(out[:2]))
            assert out[2] | out[3] << 32 == value and unwords(out[4:12]) == rand and out[12] == len(memo), n
            assert len(out) == 13 + (len(memo) + 3) // 4, n
            _eq(unwords(out[13:]), memo + b"\0" * (-len(memo) % 4), n)
        return chk
    for i, mlen in enumerate([0, 1, 2, 3, 5, 6, 21, 22, 23, 64, 80, 512]):
        key, nonce = rnd(f"an/k/{i}"), rnd(f"an/n/{i}", 12)
        value, rand, memo = int.from_bytes(rnd(f"an/v/{i}", 8), "little"), rnd(f"an/r/{i}"), rnd(f"an/m/{i}", mlen)
        ct = NC.chacha20_poly1305_seal(key, nonce, NC.serialize_plaintext(value, rand, memo))
        cs.append((f"aead note memo {mlen}", OP_AEAD_NOTE, _aead_in(key, nonce, ct), note_chk((value, rand, memo), f"memo {mlen}")))
    key, nonce, rand = rnd("an/k/x"), rnd("an/n/x", 12), rnd("an/r/x")
    seal = lambda pt: NC.chacha20_poly1305_seal(key, nonce, pt)
    head = struct.pack("<Q", 77) + rand
    for name, pt, want in (
            ("41 bytes", (head + b"\0\0")[:41], None),
            ("empty", b"", None),
            ("memo_len past the end", head + struct.pack("<H", 9) + b"12345678", None),
            ("memo_len 65535", head + b"\xff\xff" + b"x" * 500, None),
            ("memo to the last byte", head + struct.pack("<H", 9) + b"123456789", (77, rand, b"123456789")),
            ("trailing bytes", head + struct.pack("<H", 3) + b"abc" + b"trailing bytes here", (77, rand, b"abc")),
            ("trailing, empty memo", head + b"\0\0" + b"zzzzzzz", (77, rand, b""))):
        cs.append(("aead note " + name, OP_AEAD_NOTE, _aead_in(key, nonce, seal(pt)), note_chk(want, name)))
    for n in (0, 15):
        cs.append((f"aead ct of {n} bytes", OP_AEAD_NOTE, _aead_in(key, nonce, rnd("an/short", n)),
                   lambda out, n=n: _eq(bytes(out[:1]), b"\0", f"short {n}")))
    return cs


def all_cases():
    return fe_cases() + x25519_cases() + kdf_and_chacha_cases() + poly_cases() + aead_cases()


def script(cases) -> str:
    return "".join(f"{op} {unwords(w).hex()}\n" for _, op, w, _ in cases)


def check_outputs(cases, outputs):
    """outputs: one list of words per case"""
    assert len(outputs) == len(cases)
    for (name, _, _, chk), out in zip(cases, outputs):
        try:
            chk(list(out))
        except AssertionError as e:
            raise AssertionError(f"case '{name}': {e}") from None
