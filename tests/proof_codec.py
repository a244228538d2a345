"""Test-side helpers for the proof decoders (test_proof_decode_cpu.py,
test_proof_decode_abi_cpu.py, test_gpu_verify_encoded.py): the four wire
encodings written in plain Python / by the oracle, a Python statement of the
"malformed" rule of DESIGN.md section 2.9 (no library code), and the named
malformed classes of a compressed proof."""
import numpy as np

import oracle_ctypes as O

Q = O.Q
COMPRESSED, UNCOMPRESSED, SOLANA_LE, ALT_BN128_BE = 0, 1, 2, 3
FORMATS = (COMPRESSED, UNCOMPRESSED, SOLANA_LE, ALT_BN128_BE)
LEN = {COMPRESSED: 128, UNCOMPRESSED: 256, SOLANA_LE: 256, ALT_BN128_BE: 256}
INV82 = pow(82, Q - 2, Q)
TWIST_B = (27 * INV82 % Q, (-3 * INV82) % Q)  # 3 / (9 + u)


def ints(p):
    p = np.asarray(p, np.uint64)
    return [O.limbs_to_int(p[k:k + 4]) for k in range(0, len(p), 4)]


def limbs(vals):
    return np.concatenate([O.int_to_limbs(v) for v in vals]).astype(np.uint64)


def oracle_ser(p, compress):
    p = np.ascontiguousarray(p, np.uint64)
    g2 = p.size == 16
    out = np.zeros((64 if g2 else 32) * (1 if compress else 2), np.uint8)
    (O.lib().oracle_g2_serialize if g2 else O.lib().oracle_g1_serialize)(O.P(p), 1 if compress else 0, O.P(out))
    return out.tobytes()


def oracle_de(raw, compress, g2):
    """(ok, point) by oracle_g1/g2_deserialize"""
    buf = np.frombuffer(bytes(raw), np.uint8).copy()
    out = np.zeros(16 if g2 else 8, np.uint64)
    ok = (O.lib().oracle_g2_deserialize if g2 else O.lib().oracle_g1_deserialize)(O.P(buf), 1 if compress else 0,
                                                                                    O.P(out))
    return ok == 1, out


def neg_g1(p):
    x, y = ints(p)
    return limbs([x, (Q - y) % Q]) if (x or y) else np.zeros(8, np.uint64)


def neg_g2(p):
    v = ints(p)
    return limbs([v[0], v[1], (Q - v[2]) % Q, (Q - v[3]) % Q]) if any(v) else np.zeros(16, np.uint64)


def encode(fmt, a, b, c) -> bytes:
    """The wire form of canonical points, without the library: the arkworks
    forms by the oracle's serializer, the two 256-byte forms written out here."""
    if fmt in (COMPRESSED, UNCOMPRESSED):
        return b"".join(oracle_ser(p, fmt == COMPRESSED) for p in (a, b, c))
    (ax, ay), bv, (cx, cy) = ints(a), ints(b), ints(c)
    ay = (Q - ay) % Q  # -A
    if fmt == SOLANA_LE:
        return b"".join(v.to_bytes(32, "little") for v in (ax, ay, *bv, cx, cy))
    return b"".join(v.to_bytes(32, "big") for v in (ax, ay, bv[1], bv[0], bv[3], bv[2], cx, cy))


def fq2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def g1_x_has_root(x):
    rhs = (x * x * x + 3) % Q
    return rhs == 0 or pow(rhs, (Q - 1) // 2, Q) == 1


def g2_x_has_root(x):
    x3 = fq2_mul(fq2_mul(x, x), x)
    rhs = ((x3[0] + TWIST_B[0]) % Q, (x3[1] + TWIST_B[1]) % Q)
    norm = (rhs[0] * rhs[0] + rhs[1] * rhs[1]) % Q  # a square in Fq2 iff its norm is one in Fq
    return norm == 0 or pow(norm, (Q - 1) // 2, Q) == 1


def is_malformed(fmt, raw) -> bool:
    """The rule of DESIGN.md section 2.9 in plain Python."""
    raw = bytes(raw)
    if len(raw) != LEN[fmt]:
        return True
    if fmt == COMPRESSED:
        for off, n in ((0, 1), (32, 2), (96, 1)):
            body = bytearray(raw[off:off + 32 * n])
            flags = body[-1] & 0xC0
            body[-1] &= 0x3F
            if flags & 0x40:
                if flags & 0x80 or any(body):
                    return True
                continue
            xs = [int.from_bytes(body[32 * k:32 * k + 32], "little") for k in range(n)]
            if any(v >= Q for v in xs):
                return True
            if not (g1_x_has_root(xs[0]) if n == 1 else g2_x_has_root(tuple(xs))):
                return True
        return False
    if fmt == UNCOMPRESSED:
        for off, n in ((0, 2), (64, 4), (192, 2)):
            body = bytearray(raw[off:off + 32 * n])
            flags = body[-1] & 0xC0
            body[-1] &= 0x3F
            if flags & 0x40 and (flags & 0x80 or any(body)):
                return True
            if any(int.from_bytes(body[32 * k:32 * k + 32], "little") >= Q for k in range(n)):
                return True
        return False
    order = "little" if fmt == SOLANA_LE else "big"
    return any(int.from_bytes(raw[32 * k:32 * k + 32], order) >= Q for k in range(8))


def fq2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = fq2_mul(r, a)
        a = fq2_mul(a, a)
        e >>= 1
    return r


def twist_point_off_subgroup():
    """a point of the twist with x = k + u for the first k that has one: the
    twist's cofactor is ~2^254, so it lies outside the order-r subgroup"""
    for k in range(1, 100):
        if not g2_x_has_root((k, 1)):
            continue
        x3 = fq2_mul(fq2_mul((k, 1), (k, 1)), (k, 1))
        a = ((x3[0] + TWIST_B[0]) % Q, (x3[1] + TWIST_B[1]) % Q)
        a1 = fq2_pow(a, (Q - 3) // 4)  # Adj & Rodriguez-Henriquez, Algorithm 9
        alpha, x0 = fq2_mul(fq2_mul(a1, a1), a), fq2_mul(a1, a)
        y = ((-x0[1]) % Q, x0[0]) if alpha == (Q - 1, 0) else \
            fq2_mul(fq2_pow(((1 + alpha[0]) % Q, alpha[1]), (Q - 1) // 2), x0)
        assert fq2_mul(y, y) == a
        return limbs([k, 1, y[0], y[1]])
    raise AssertionError("no twist point found")


def non_residue_x_g1():
    return next(x for x in range(1, 100) if not g1_x_has_root(x))


def non_residue_x_g2():
    return next((k, 1) for k in range(1, 100) if not g2_x_has_root((k, 1)))


def patch(raw, off, data):
    raw = bytearray(raw)
    raw[off:off + len(data)] = data
    return bytes(raw)


def le32(v, flags=0):
    b = bytearray(v.to_bytes(32, "little"))
    b[31] |= flags
    return bytes(b)


def malformed_compressed(good):
    """{class name: a malformed variant of the well-formed compressed proof
    `good`}: every class of the rule, on A, on both halves of B's x and on C."""
    out = {}
    for name, off in (("a", 0), ("b", 64), ("c", 96)):  # off: the 32-byte field that carries the point's flags
        fld = good[off:off + 32]
        p0 = 32 if name == "b" else off
        zero = bytes(off + 32 - p0)
        out[f"{name}_inf_flag_on_point"] = patch(good, off + 31, bytes([fld[31] & 0x3F | 0x40]))
        out[f"{name}_both_flags_on_point"] = patch(good, off + 31, bytes([fld[31] | 0xC0]))
        out[f"{name}_both_flags_on_zero"] = patch(patch(good, p0, zero), off + 31, b"\xC0")
        out[f"{name}_inf_stray_bit"] = patch(patch(good, p0, zero), p0 + 5, b"\x10")[:off + 31] + b"\x40" + \
            good[off + 32:]
        for v, tag in ((Q, "q"), (Q + 1, "q_plus_1"), (2**254 - 1, "2_254_minus_1")):
            out[f"{name}_x_{tag}"] = patch(good, off, le32(v))
    out["b_c0_x_q"] = patch(good, 32, le32(Q))
    out["b_c0_x_q_plus_1"] = patch(good, 32, le32(Q + 1))
    out["b_c0_x_2_256_minus_1"] = patch(good, 32, le32(2**256 - 1))
    x1 = non_residue_x_g1()
    out["a_non_residue"] = patch(good, 0, le32(x1))
    out["c_non_residue"] = patch(good, 96, le32(x1, 0x80))
    x2 = non_residue_x_g2()
    out["b_non_residue"] = patch(good, 32, le32(x2[0]) + le32(x2[1]))
    return out


def sample_proofs(seed, n):
    """n triples of oracle points (A, C on G1; B in G2's subgroup): well-formed
    and valid as points, not proofs of anything"""
    g1 = O.gen_points_g1(seed, 2 * n)
    g2 = O.gen_points_g2(seed + 1, n)
    return [(g1[2 * i], g2[i], g1[2 * i + 1]) for i in range(n)]
