"""Cases for the op table of tests/device/ed25519_ops.h, shared by the host
check (test_ed25519_cpu.py) and the device probe (test_gpu_ed25519.py).  A case
is (name, op, input words, check); check(output words) asserts against Python
integers, hashlib, the golden vectors (libcrypto's) or the model
(zelana_amd/ed25519.py)."""
import hashlib
import json
import os
import struct

from zelana_amd import ed25519 as E

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ed25519_vectors.json")
P, L = E.P, E.L
ED_IN, ED_OUT = 112, 24
(OP_SHA512, OP_SC_REDUCE, OP_SC_CANONICAL, OP_DECOMPRESS, OP_ADD, OP_DBL, OP_COMPRESS, OP_VERIFY_CORE, OP_VERIFY,
 OP_SCALAR_MUL) = range(1, 11)
SHA_LENS = [0, 1, 111, 112, 127, 128, 129, 239, 240, 256]
SHIFT = [(51 * i + 1) // 2 for i in range(10)]
BITS = [26 if i % 2 == 0 else 25 for i in range(10)]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def rnd(tag: str, n: int = 32) -> bytes:
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha256(f"ed/{tag}/{i}".encode()).digest()
        i += 1
    return out[:n]


def words(b: bytes) -> list:
    b = bytes(b) + b"\0" * (-len(b) % 4)
    return list(struct.unpack(f"<{len(b) // 4}I", b))


def unwords(w) -> bytes:
    return struct.pack(f"<{len(w)}I", *w)


def le32(v: int) -> bytes:
    return v.to_bytes(32, "little")


def fe_limbs(v: int) -> list:
    assert 0 <= v < 1 << 255
    return [(v >> s) & ((1 << b) - 1) for s, b in zip(SHIFT, BITS)]


def _eq(got, want, name):
    assert got == want, (name, got.hex()[:64], want.hex()[:64])


def sha_cases():
    cs = []
    for n in SHA_LENS:
        m = rnd(f"sha/{n}", n)
        cs.append((f"sha512 len {n}", OP_SHA512, [n] + words(m),
                   lambda out, want=hashlib.sha512(m).digest(), nm=f"sha {n}": _eq(unwords(out), want, nm)))
    return cs


REDUCE_VALUES = [0, L - 1, L, L + 1, 2**252, 2**512 - 1, 2**260 - 1, 2**260, (L << 259) - 1] + \
    [int.from_bytes(rnd(f"red/{i}", 64), "little") for i in range(8)]
CANONICAL_VALUES = [0, L - 1, L, L + 1, 2**256 - 1, 2**252]


def scalar_cases():
    cs = []
    for i, v in enumerate(REDUCE_VALUES):
        cs.append((f"sc_reduce512 {i}", OP_SC_REDUCE, words(v.to_bytes(64, "little")),
                   lambda out, v=v, nm=f"reduce {i}": _eq(unwords(out), le32(v % L), nm)))
    for i, v in enumerate(CANONICAL_VALUES):
        def chk(out, v=v, nm=f"canonical {i}"):
            assert list(out) == [1 if v < L else 0], nm
        cs.append((f"sc_is_canonical {i}", OP_SC_CANONICAL, words(le32(v)), chk))
    return cs


def decompress_inputs():
    """[(name, 32 bytes)]: the golden edge keys, the named edges and random y
    under both sign bits"""
    out = [("golden " + c["name"], bytes.fromhex(c["public_key"])) for c in golden()["verify"]]
    for name, y in (("y = 0", 0), ("y = 1", 1), ("y = p - 1", P - 1), ("y = p", P), ("y = p + 1", P + 1),
                    ("y = 2^255 - 1", 2**255 - 1), ("y = 2^255 - 20", 2**255 - 20)):
        out += [(name, le32(y)), (name + ", sign set", le32(y | 1 << 255))]
    for i in range(24):
        y = int.from_bytes(rnd(f"dec/{i}"), "little")
        out.append((f"random {i}", le32(y)))
    return out


def decompress_cases():
    cs = []
    for name, b in decompress_inputs():
        def chk(out, b=b, nm=name):
            p = E.decompress(b)
            if p is None:
                assert list(out) == [0], (nm, "the model refuses these bytes", list(out[:1]))
                return
            assert out[0] == 1, (nm, "the model accepts these bytes")
            x, y = E.affine(p)
            _eq(unwords(out[1:9]), le32(x), nm + " x")
            _eq(unwords(out[9:17]), le32(y), nm + " y")
            assert out[17] == 1, (nm, "T is not X Y / Z")
        cs.append(("decompress " + name, OP_DECOMPRESS, words(b), chk))
    return cs


def some_points():
    """[(name, compressed bytes)] that decompress: the base point and multiples,
    the identity, the points of order 2 and 8, random points"""
    g = golden()["verify"]
    order8 = next(bytes.fromhex(c["public_key"]) for c in g if c["name"].startswith("A of order 8"))
    pts = [("B", E.compress(E.BASE)), ("identity", le32(1)), ("order 2", le32(P - 1)), ("order 8", order8),
           ("identity, y = p + 1", le32(P + 1))]
    for i in range(4):
        k = int.from_bytes(rnd(f"pt/{i}"), "little")
        pts.append((f"[k{i}]B", E.compress(E.point_mul(k, E.BASE))))
    pts.append(("B + order 8", E.compress(E.point_add(E.BASE, E.decompress(order8)))))
    return pts


def group_cases():
    cs, pts = [], some_points()
    neg = lambda b: b[:31] + bytes([b[31] ^ 0x80])
    pairs = [(n1 + " + " + n2, b1, b2) for n1, b1 in pts for n2, b2 in pts]        # P + P on the diagonal
    pairs += [(n + " + its negative", b, neg(b)) for n, b in pts]
    for name, b1, b2 in pairs:
        want = E.compress(E.point_add(E.decompress(b1), E.decompress(b2)))
        cs.append(("add " + name, OP_ADD, words(b1) + words(b2), lambda out, want=want, nm=name: _eq(unwords(out), want, nm)))
    for name, b in pts:
        pt = E.decompress(b)
        want = E.compress(E.point_add(pt, pt))
        cs.append(("dbl " + name, OP_DBL, words(b), lambda out, want=want, nm=name: _eq(unwords(out), want, "dbl " + nm)))
        # compress from projective limbs: Z != 1, and coordinates that are not reduced where they fit 255 bits
        x, y = E.affine(pt)
        for j, z in enumerate([1, 2, P - 1, int.from_bytes(rnd(f"z/{name}"), "little") % P]):
            coords = [x * z % P, y * z % P, z % P]
            coords = [c + P if j == 3 and c + P < 2**255 else c for c in coords]
            cs.append((f"compress {name} z{j}", OP_COMPRESS, sum((fe_limbs(c) for c in coords), []),
                       lambda out, want=E.compress(pt), nm=f"compress {name} z{j}": _eq(unwords(out), want, nm)))
    return cs


def scalar_mul_cases():
    cs = []
    pts = some_points()
    scalars = [0, 1, 15, 16, L - 1, L, 2**256 - 1] + [int.from_bytes(rnd(f"sm/{i}"), "little") for i in range(3)]
    for i, s in enumerate(scalars):
        k = scalars[(3 * i + 1) % len(scalars)]
        name, q = pts[i % len(pts)]
        want = E.compress(E.point_add(E.point_mul(s, E.BASE), E.point_mul(k, E.decompress(q))))
        cs.append((f"scalar_mul {i} {name}", OP_SCALAR_MUL, words(le32(s)) + words(le32(k)) + words(q),
                   lambda out, want=want, nm=f"scalar_mul {i}": _eq(unwords(out), want, nm)))
    return cs


def golden_triples():
    """[(name, pk, msg, sig, libcrypto says ok, reason by construction)] of both sections"""
    g = golden()
    out = [(f"sign len {c['len']}", bytes.fromhex(c["public_key"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["signature"]),
            True, E.SIG_OK) for c in g["sign"]]
    out += [(c["name"], bytes.fromhex(c["public_key"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["signature"]),
             c["ok"], c["reason"]) for c in g["verify"]]
    return out


def verify_cases():
    cs = []
    for name, pk, msg, sig, ok, reason in golden_triples():
        def chk(out, ok=ok, reason=reason, nm=name):
            assert (out[0] == E.SIG_OK) == ok, (nm, "libcrypto's verdict", out[0])
            assert list(out) == [reason], (nm, "the reason", out[0], reason)
        cs.append(("verify " + name, OP_VERIFY, words(pk) + words(sig) + [len(msg)] + words(msg), chk))
        k, s = E.challenge(sig[:32], pk, msg), int.from_bytes(sig[32:], "little")
        # the core takes s as it comes: the equation alone, with k from hashlib
        a = E.decompress(pk)
        want = 2 if a is None else int(E.verify_core(sig[:32], a, k, s))
        if reason != E.SIG_BAD_S:
            assert want == {E.SIG_OK: 1, E.SIG_MISMATCH: 0, E.SIG_BAD_PUBKEY: 2}[reason], name
        def chk_core(out, want=want, nm=name):
            assert list(out) == [want], (nm, "verify_core", list(out), want)
        cs.append(("verify_core " + name, OP_VERIFY_CORE, words(sig[:32]) + words(pk) + words(le32(k)) + words(sig[32:]),
                   chk_core))
    return cs


def all_cases():
    return sha_cases() + scalar_cases() + decompress_cases() + group_cases() + scalar_mul_cases() + verify_cases()


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
