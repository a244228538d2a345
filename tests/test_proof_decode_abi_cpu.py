"""CPU: zkmi_proof_decode / zkmi_proof_encoded_len through the C ABI (host
code, no GPU): against the oracle's deserializers on well-formed encodings and
on the reference's two golden proofs, as the exact inverse of the library's
three encoders, against prover.proof_points_from_solana_bytes, and on the
encodings where the rule of DESIGN.md section 2.9 is stricter than the oracle
(those must come back malformed)."""
import base64
import ctypes
import json
import os

import numpy as np
import pytest

import oracle_ctypes as O
import proof_codec as PC
from test_pairing import ref_proof

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EINVAL, EPOINT = -1, -5
Q = PC.Q
u8p = ctypes.POINTER(ctypes.c_uint8)
SEED_X = 20261020  # the draws of test_root_and_non_residue_draws (checked there against the oracle)


def L():
    from zelana_amd._lib import lib
    return lib()


def decode(fmt, raw):
    """(rc, a, b, c) of zkmi_proof_decode"""
    buf = np.frombuffer(bytes(raw), np.uint8).copy()
    a, b, c = np.full(8, 7, np.uint64), np.full(16, 7, np.uint64), np.full(8, 7, np.uint64)
    rc = L().zkmi_proof_decode(fmt, buf.ctypes.data_as(u8p), buf.size, O.P(a), O.P(b), O.P(c))
    if rc:
        assert not a.any() and not b.any() and not c.any(), "a failed decode leaves zeroed points"
    return rc, a, b, c


def lib_encode(fmt, a, b, c) -> bytes:
    from zelana_amd import gpu
    return {PC.COMPRESSED: gpu.proof_serialize_compressed, PC.SOLANA_LE: gpu.proof_to_solana_bytes,
            PC.ALT_BN128_BE: gpu.proof_to_alt_bn128_bytes}[fmt](a, b, c)


@pytest.fixture(scope="module")
def samples():
    pts = PC.sample_proofs(777, 32)
    za, zb = np.zeros(8, np.uint64), np.zeros(16, np.uint64)
    a, b, c = pts[0]
    pts[1:4] = [(za, b, c), (a, zb, c), (a, b, za)]  # infinities ride along
    pts[4] = (PC.neg_g1(a), PC.neg_g2(b), PC.neg_g1(c))
    return pts


def test_encoded_len():
    assert [L().zkmi_proof_encoded_len(f) for f in (0, 1, 2, 3)] == [128, 256, 256, 256]
    assert L().zkmi_proof_encoded_len(4) == 0 and L().zkmi_proof_encoded_len(-1) == 0


def test_matches_oracle_deserializers(samples):
    for a, b, c in samples:
        for fmt, comp in ((PC.COMPRESSED, True), (PC.UNCOMPRESSED, False)):
            raw = PC.encode(fmt, a, b, c)
            na, nb_ = (32, 64) if comp else (64, 128)
            want = [PC.oracle_de(raw[:na], comp, False), PC.oracle_de(raw[na:na + nb_], comp, True),
                    PC.oracle_de(raw[na + nb_:], comp, False)]
            assert all(ok for ok, _ in want)
            rc, da, db, dc = decode(fmt, raw)
            assert rc == 0
            for got, (_, w), src in zip((da, db, dc), want, (a, b, c)):
                assert np.array_equal(got, w) and np.array_equal(got, np.asarray(src, np.uint64))


def test_golden_compressed_proof():
    raw = base64.b64decode(json.load(open(os.path.join(GOLD, "ref_l2_proof.json")))["proof"])
    assert len(raw) == 128
    rc, a, b, c = decode(PC.COMPRESSED, raw)
    assert rc == 0
    for got, (ok, w) in zip((a, b, c), (PC.oracle_de(raw[:32], True, False), PC.oracle_de(raw[32:96], True, True),
                                        PC.oracle_de(raw[96:], True, False))):
        assert ok and np.array_equal(got, w)
    assert lib_encode(PC.COMPRESSED, a, b, c) == raw


def test_golden_uncompressed_proof():
    comp = json.load(open(os.path.join(GOLD, "ref_proof_for_onchain.json")))["proof_components"]
    raw = bytes(comp["pi_a"]) + bytes(comp["pi_b"]) + bytes(comp["pi_c"])
    assert len(raw) == 256
    rc, a, b, c = decode(PC.UNCOMPRESSED, raw)
    (wa, wb, wc), _ = ref_proof()  # the oracle's reading of the same file
    assert rc == 0 and np.array_equal(a, wa) and np.array_equal(b, wb) and np.array_equal(c, wc)


@pytest.mark.parametrize("fmt", [PC.COMPRESSED, PC.SOLANA_LE, PC.ALT_BN128_BE])
def test_inverse_of_the_encoders(samples, fmt):
    from zelana_amd.prover import proof_points_from_solana_bytes
    for a, b, c in samples:
        raw = lib_encode(fmt, a, b, c)
        assert raw == PC.encode(fmt, a, b, c)  # the encoder itself, against the plain-Python / oracle form
        rc, da, db, dc = decode(fmt, raw)
        assert rc == 0 and np.array_equal(da, a) and np.array_equal(db, b) and np.array_equal(dc, c)
        if fmt == PC.SOLANA_LE:
            pa, pb, pc = proof_points_from_solana_bytes(raw)
            assert np.array_equal(da, pa) and np.array_equal(db, pb) and np.array_equal(dc, pc)


def test_solana_equals_python_decoder_on_arbitrary_words():
    """wherever all coordinates are < q the two decoders agree, whether or not
    the words are points (the verdict then is EPOINT, the words zeroed: compare
    through the well-formedness verdict and the re-encoding)"""
    from zelana_amd import gpu
    from zelana_amd.prover import proof_points_from_solana_bytes
    rng = np.random.default_rng(99)
    for _ in range(64):
        vals = [int.from_bytes(rng.bytes(32), "little") % Q for _ in range(8)]
        raw = b"".join(v.to_bytes(32, "little") for v in vals)
        rc, *_ = decode(PC.SOLANA_LE, raw)
        assert rc == EPOINT  # well-formed; random words are no curve points
        pa, pb, pc = proof_points_from_solana_bytes(raw)
        assert gpu.proof_to_solana_bytes(pa, pb, pc) == raw


def test_accepted_compressed_strings_reserialize(samples):
    seen = 0
    for a, b, c in samples[:8]:
        good = PC.encode(PC.COMPRESSED, a, b, c)
        variants = [good] + [PC.patch(good, off, bytes([good[off] ^ 0x80])) for off in (31, 95, 127)]
        variants += list(PC.malformed_compressed(good).values())
        for raw in variants:
            rc, da, db, dc = decode(PC.COMPRESSED, raw)
            assert (rc == EINVAL) == PC.is_malformed(PC.COMPRESSED, raw)
            if rc == 0:
                assert lib_encode(PC.COMPRESSED, da, db, dc) == raw
                seen += 1
    assert seen >= 8


def test_stricter_than_the_oracle(samples):
    """The oracle (like k_decode_* on key load) takes the infinity flag alone;
    proof decoding wants every other bit zero.  Bit 7 of an uncompressed point
    is ignored by both."""
    a, b, c = samples[0]
    comp, unc = PC.encode(PC.COMPRESSED, a, b, c), PC.encode(PC.UNCOMPRESSED, a, b, c)
    for fmt, raw, offs in ((PC.COMPRESSED, comp, ((31, 0, 32, False), (95, 32, 64, True), (127, 96, 32, False))),
                           (PC.UNCOMPRESSED, unc, ((63, 0, 64, False), (191, 64, 128, True), (255, 192, 64, False)))):
        for off, p0, n, g2 in offs:
            for flags in (0x40, 0xC0):  # infinity flag on a non-zero body / with bit 7
                bad = PC.patch(raw, off, bytes([raw[off] & 0x3F | flags]))
                ok, pt = PC.oracle_de(bad[p0:p0 + n], fmt == PC.COMPRESSED, g2)
                assert ok and not pt.any()  # the oracle reads infinity
                assert decode(fmt, bad)[0] == EINVAL
            zero_c0 = PC.patch(PC.patch(raw, p0, bytes(n)), off, b"\xC0")
            assert PC.oracle_de(zero_c0[p0:p0 + n], fmt == PC.COMPRESSED, g2)[0]
            assert decode(fmt, zero_c0)[0] == EINVAL
            inf = PC.patch(PC.patch(raw, p0, bytes(n)), off, b"\x40")  # the one accepted infinity
            rc, da, db, dc = decode(fmt, inf)
            assert rc == 0 and not (db if g2 else da if p0 == 0 else dc).any()
    for off in (63, 191, 255):
        rc, da, db, dc = decode(PC.UNCOMPRESSED, PC.patch(unc, off, bytes([unc[off] | 0x80])))
        assert rc == 0 and np.array_equal(da, a) and np.array_equal(db, b) and np.array_equal(dc, c)


def test_malformed_and_invalid_are_told_apart(samples):
    a, b, c = samples[0]
    for fmt in PC.FORMATS:
        raw = PC.encode(fmt, a, b, c)
        assert decode(fmt, raw)[0] == 0
        assert decode(fmt, raw[:-1])[0] == EINVAL and decode(fmt, raw + b"\0")[0] == EINVAL
        assert decode(7, raw)[0] == EINVAL
        # B outside the subgroup: well-formed in every format, an invalid point
        assert decode(fmt, PC.encode(fmt, a, PC.twist_point_off_subgroup(), c))[0] == EPOINT
        if fmt != PC.COMPRESSED:  # (a compressed point is on the curve by construction)
            order = "big" if fmt == PC.ALT_BN128_BE else "little"
            for k in range(8):
                v = int.from_bytes(raw[32 * k:32 * k + 32], order)
                assert decode(fmt, PC.patch(raw, 32 * k, ((v + 1) % Q).to_bytes(32, order)))[0] == EPOINT
                assert decode(fmt, PC.patch(raw, 32 * k, Q.to_bytes(32, order)))[0] == EINVAL
    for raw in PC.malformed_compressed(PC.encode(PC.COMPRESSED, a, b, c)).values():
        assert decode(PC.COMPRESSED, raw)[0] == EINVAL


def test_root_and_non_residue_draws(samples):
    """64 seeded x < q: both outcomes of the square root occur often (expected
    32 each), the oracle and the rule agree on which, and zkmi_proof_decode
    follows them on A and on C."""
    a, b, c = samples[0]
    good = PC.encode(PC.COMPRESSED, a, b, c)
    rng = np.random.default_rng(SEED_X)
    roots = 0
    for t in range(64):
        x = int.from_bytes(rng.bytes(32), "little") % Q
        has = PC.oracle_de(PC.le32(x), True, False)[0]
        assert has == PC.g1_x_has_root(x)
        roots += has
        raw = PC.patch(good, 96 if t & 1 else 0, PC.le32(x, 0x80 if t & 2 else 0))
        assert decode(PC.COMPRESSED, raw)[0] == (0 if has else EINVAL)
    assert roots >= 16 and 64 - roots >= 16, roots
    g2_roots = 0
    for t in range(64):  # the same for B's x (the oracle's G2 reader also checks the subgroup, so the rule alone)
        x = tuple(int.from_bytes(rng.bytes(32), "little") % Q for _ in range(2))
        has = PC.g2_x_has_root(x)
        g2_roots += has
        rc = decode(PC.COMPRESSED, PC.patch(good, 32, PC.le32(x[0]) + PC.le32(x[1], 0x80 if t & 1 else 0)))[0]
        assert rc == (EPOINT if has else EINVAL)  # a random twist point is outside the subgroup
    assert g2_roots >= 16 and 64 - g2_roots >= 16, g2_roots
