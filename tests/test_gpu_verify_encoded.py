"""Groth16 verification from wire bytes, decoded on the GPU
(zkmi_groth16_verify_many_encoded / _each_encoded / zkmi_proofs_decode,
DESIGN.md section 2.9): every verdict equals zkmi_groth16_verify's on
zkmi_proof_decode's points, every decoded word and status equals the host
decoder's, and the stats equal those of the point-taking calls on the same
proofs.  Proofs and key: test_gpu_verify_many's.  Sizes: 22 is the first size
whose 3 nb + 1 pairs pass one block of k_miller; 64 / 65 straddle the 64-lane
block of the decode kernels (at 65 the compressed decoder's B, A and C lane
ranges all start inside a wave); 131 spans more than two blocks."""
import numpy as np
import pytest

import oracle_ctypes as O
import proof_codec as PC
from test_gpu_verify_many import ctx, env, host, twist_point_outside_subgroup  # noqa: F401  (ctx, env: fixtures)

pytestmark = pytest.mark.gpu

Q, R = O.Q, O.R
NB = 65
FMTS = [PC.COMPRESSED, PC.UNCOMPRESSED, PC.SOLANA_LE, PC.ALT_BN128_BE]


def encode(fmt, a, b, c) -> bytes:
    """the library's encoders; the oracle's serializer for the format that has none"""
    from zelana_amd import gpu
    if fmt == PC.UNCOMPRESSED:
        return PC.encode(fmt, a, b, c)
    return {PC.COMPRESSED: gpu.proof_serialize_compressed, PC.SOLANA_LE: gpu.proof_to_solana_bytes,
            PC.ALT_BN128_BE: gpu.proof_to_alt_bn128_bytes}[fmt](a, b, c)


@pytest.fixture(scope="module")
def raws(env):
    """{fmt: the encodings of env's proofs}"""
    return {fmt: [encode(fmt, *p) for p in env["proofs"]] for fmt in FMTS}


_point_stats = {}


def point_stats(ctx, env, nb):
    """(verify_many's, verify_each's) stats of the point-taking calls on the first nb proofs, once per size"""
    from zelana_amd import gpu
    if nb not in _point_stats:
        vm, sm = gpu.groth16_verify_many(ctx, env["vk"], env["proofs"][:nb], env["inputs"][:nb])
        ve, se = gpu.groth16_verify_each(ctx, env["vk"], env["proofs"][:nb], env["inputs"][:nb])
        assert vm == ve == [True] * nb
        _point_stats[nb] = (sm, se)
    return _point_stats[nb]


def host_decode(fmt, raw):
    """(status, a, b, c) of zkmi_proof_decode: the rows of a failed decode are zero"""
    from zelana_amd import gpu
    try:
        return (0,) + tuple(gpu.proof_decode(fmt, raw))
    except gpu.ProofDecodeError as e:
        return e.status, np.zeros(8, np.uint64), np.zeros(16, np.uint64), np.zeros(8, np.uint64)


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nb", [0, 1, 22, 64, 65, 131])
def test_sizes_all_valid(ctx, env, raws, nb, fmt):
    from zelana_amd import gpu
    sm, se = point_stats(ctx, env, nb)
    valid, mal, st = gpu.groth16_verify_many_encoded(ctx, env["vk"], fmt, raws[fmt][:nb], env["inputs"][:nb])
    assert valid == [True] * nb and mal == [False] * nb and st == sm
    valid, mal, st = gpu.groth16_verify_each_encoded(ctx, env["vk"], fmt, b"".join(raws[fmt][:nb]), env["inputs"][:nb])
    assert valid == [True] * nb and mal == [False] * nb and st == se


# ------------------------------------------------------------------ 2. decode
def spoiled(fmt, raws, nb):
    """the first nb encodings with every 5th malformed (the classes in turn) and every 7th an invalid point"""
    out = list(raws[fmt][:nb])
    classes = list(PC.malformed_compressed(out[0]).keys())
    for i in range(0, nb, 5):
        if fmt == PC.COMPRESSED:
            out[i] = PC.malformed_compressed(out[i])[classes[(i // 5) % len(classes)]]
        else:
            order = "big" if fmt == PC.ALT_BN128_BE else "little"
            out[i] = PC.patch(out[i], 32 * ((i // 5) % 8), (Q + i).to_bytes(32, order))
    off = twist_point_outside_subgroup()
    for i in range(3, nb, 7):
        if i % 5 == 0:
            continue
        a, b, c = host_decode(fmt, out[i])[1:]
        if fmt == PC.COMPRESSED or i % 2:
            out[i] = encode(fmt, a, off, c)
        else:  # off the curve: only a format that carries y can say so
            out[i] = encode(fmt, a, b, np.concatenate([c[:4], c[4:] ^ np.uint64(1)]))
    return out


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nb", [65, 131])
def test_proofs_decode_equals_host_decode(ctx, raws, nb, fmt):
    from zelana_amd import gpu
    enc = spoiled(fmt, raws, nb)
    a, b, c, status = gpu.proofs_decode(ctx, fmt, enc)
    want = [host_decode(fmt, r) for r in enc]
    assert [int(s) for s in status] == [w[0] for w in want]
    assert {0, 1, 2} <= set(int(s) for s in status)
    for i, (_, wa, wb, wc) in enumerate(want):
        assert np.array_equal(a[i], wa) and np.array_equal(b[i], wb) and np.array_equal(c[i], wc), i
    assert all(np.array_equal(gpu.proofs_decode(ctx, fmt, b"")[k], np.zeros((0, n), np.uint64))
               for k, n in ((0, 8), (1, 16), (2, 8)))


# ------------------------------------------------------------------ 3. one malformed proof
def one_malformed(ctx, env, fmt, base, bad_raw):
    from zelana_amd import gpu
    for pos in (0, 32, 64):
        enc = list(base)
        enc[pos] = bad_raw(enc[pos])
        want = [i != pos for i in range(NB)]
        for fn in (gpu.groth16_verify_many_encoded, gpu.groth16_verify_each_encoded):
            valid, mal, st = fn(ctx, env["vk"], fmt, enc, env["inputs"][:NB])
            assert valid == want, (fn.__name__, pos)
            assert mal == [i == pos for i in range(NB)], (fn.__name__, pos)
            assert st["invalid_points"] == 1, (fn.__name__, pos, st)


_CLASSES = sorted(PC.malformed_compressed(bytes(128)).keys())


@pytest.mark.parametrize("cls", _CLASSES)
def test_malformed_compressed_at_position(ctx, env, raws, cls):
    one_malformed(ctx, env, PC.COMPRESSED, raws[PC.COMPRESSED][:NB], lambda r: PC.malformed_compressed(r)[cls])


@pytest.mark.parametrize("k", [1, 7])  # y of A, y of C
def test_solana_y_not_below_q_at_position(ctx, env, raws, k):
    one_malformed(ctx, env, PC.SOLANA_LE, raws[PC.SOLANA_LE][:NB],
                  lambda r: PC.patch(r, 32 * k, Q.to_bytes(32, "little")))


# ------------------------------------------------------------------ 4. well-formed, not valid
def test_well_formed_but_bad(ctx, env, raws):
    from zelana_amd import gpu
    enc = list(raws[PC.COMPRESSED][:NB])
    inputs = [list(i) for i in env["inputs"][:NB]]
    a, b, c = env["proofs"][10]
    sub = (a, twist_point_outside_subgroup(), c)
    enc[10] = encode(PC.COMPRESSED, *sub)
    inputs[40] = [(inputs[40][0] + 1) % R]
    want = [True] * NB
    want[10], want[40] = host(env, [sub, env["proofs"][40]], [inputs[10], inputs[40]])
    assert want[10] is False and want[40] is False
    for fn in (gpu.groth16_verify_many_encoded, gpu.groth16_verify_each_encoded):
        valid, mal, st = fn(ctx, env["vk"], PC.COMPRESSED, enc, inputs)
        assert valid == want and mal == [False] * NB and st["invalid_points"] == 1, fn.__name__


# ------------------------------------------------------------------ 5. budget, arguments
def test_budget_hands_encoded_batch_over(ctx, env, raws):
    from zelana_amd import gpu
    all_bad = [[(x[0] + 1) % R] for x in env["inputs"][:NB]]
    try:
        ctx.set_verify_probes(1)
        enc = raws[PC.COMPRESSED][:NB]
        valid, mal, st = gpu.groth16_verify_many_encoded(ctx, env["vk"], PC.COMPRESSED, enc, all_bad)
        assert valid == [False] * NB and mal == [False] * NB
        assert st == {"pairs": NB + 3, "final_exps": 1, "invalid_points": 0}
        assert gpu.groth16_verify_last(ctx) == {"gpu_decided": NB, "gpu_pairs": 3 * NB + 1, "gpu_final_exps": NB}
    finally:
        ctx.set_verify_probes(0)


def test_argument_rules(ctx, env, raws):
    from zelana_amd import ZkmiError, gpu
    enc, inputs = raws[PC.SOLANA_LE][:3], [list(i) for i in env["inputs"][:3]]
    with pytest.raises(ValueError):
        gpu.groth16_verify_many_encoded(ctx, env["vk"], 9, enc, inputs)  # unknown format
    with pytest.raises(ValueError):
        gpu.groth16_verify_each_encoded(ctx, env["vk"], PC.SOLANA_LE, [enc[0][:255]], inputs[:1])
    inputs[1] = [R]
    for fn in (gpu.groth16_verify_many_encoded, gpu.groth16_verify_each_encoded):
        with pytest.raises(ZkmiError):
            fn(ctx, env["vk"], PC.SOLANA_LE, enc, inputs)
    c2 = gpu.Context(0)
    try:
        with pytest.raises(ZkmiError):  # a key of another context
            gpu.groth16_verify_many_encoded(c2, env["vk"], PC.SOLANA_LE, enc, env["inputs"][:3])
    finally:
        c2.close()


# ------------------------------------------------------------------ 6. golden
def test_golden_uncompressed_proof_from_bytes(ctx):
    import json
    import os

    from test_pairing import ref_proof, ref_vk
    from test_verify_cpu import compressed_vk
    from zelana_amd import gpu
    comp = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_proof_for_onchain.json")))
    raw = b"".join(bytes(comp["proof_components"][k]) for k in ("pi_a", "pi_b", "pi_c"))
    vk = gpu.VerifyingKey(ctx, compressed_vk(ref_vk()))
    _, x = ref_proof()
    valid, mal, _ = gpu.groth16_verify_each_encoded(ctx, vk, PC.UNCOMPRESSED, [raw, raw], [[x], [x + 1]])
    assert valid == [True, False] and mal == [False, False]
    assert gpu.groth16_verify_many_encoded(ctx, vk, PC.UNCOMPRESSED, raw, [[x]])[0] == [True]
    vk.close()


# ------------------------------------------------------------------ 7. Python surface
def test_prover_surface(ctx, env, raws):
    from zelana_amd import gpu
    from zelana_amd.prover import BatchProof, BatchPublicInputs, Groth16Prover
    prover = Groth16Prover(ctx, env["pk"], env["vkb"], circuit=lambda i, w: None)
    a, b, c = env["proofs"][0]
    bp = BatchProof(BatchPublicInputs(batch_id=3), gpu.proof_to_solana_bytes(a, b, c), 0, a, b, c)
    back = Groth16Prover.import_proof_json(Groth16Prover.export_proof_json(bp), bp.public_inputs)
    assert back.proof_bytes == bp.proof_bytes and back.public_inputs == bp.public_inputs
    assert np.array_equal(back.a, a) and np.array_equal(back.b, b) and np.array_equal(back.c, c)
    assert prover.verify_pairing(back, env["inputs"][0]) and prover.verify_many([back], [env["inputs"][0]]) == [True]
    import base64
    import json
    bad = PC.patch(gpu.proof_serialize_compressed(a, b, c), 0, PC.le32(Q))  # A's x = q
    with pytest.raises(gpu.ProofDecodeError):
        Groth16Prover.import_proof_json(json.dumps({"proof": base64.b64encode(bad).decode()}), bp.public_inputs)
    enc, ins = list(raws[PC.SOLANA_LE][:6]), [list(i) for i in env["inputs"][:6]]
    enc[2] = PC.patch(enc[2], 200, bytes([enc[2][200] ^ 1]))
    ins[4] = [ins[4][0] + 1]
    want = [True, True, False, True, False, True]
    assert prover.verify_many_encoded(gpu.PROOF_SOLANA_LE, enc, ins) == want
    assert prover.verify_many_encoded(gpu.PROOF_SOLANA_LE, enc, ins, each=True) == want
    assert prover.verify_many_encoded(gpu.PROOF_ARK_COMPRESSED, [], []) == []


def test_batch_worker_verify_results(ctx):
    """three ProofResults of a reduced-shape ZBatchProver (test_gpu_zbatch's):
    untouched, a flipped proof byte, a truncated witness"""
    import copy
    import ctypes

    from zelana_amd import batch_worker as BW
    from zelana_amd import gpu, zbatch as Z
    shape = dict(max_transfers=1, max_withdrawals=1, max_shielded=1, depth=2)
    d = Z.synthetic_batch(2, 1, seed=102)
    cs, z, _ = Z.build(d, **shape)
    st, keep = O.make_r1cs(cs)
    opk = O.lib().oracle_groth16_setup(ctypes.byref(st), O.Rng(0).h, 8)
    size = O.lib().oracle_pk_serialize(opk, 1, None, 0)
    buf = np.zeros(size, np.uint8)
    O.lib().oracle_pk_serialize(opk, 1, buf.ctypes.data, size)
    pk = gpu.ProvingKey(ctx, buf.tobytes(), True)
    w = BW.ZBatchProver(ctx, d, pk=pk, **shape)
    vk = gpu.VerifyingKey(ctx, pk.vk_bytes())
    res = w.generate_batch_proof(d)
    flipped, cut, big, short = (copy.copy(res) for _ in range(4))
    flipped.proof_bytes = PC.patch(res.proof_bytes, 70, bytes([res.proof_bytes[70] ^ 4]))
    cut.public_witness_bytes = res.public_witness_bytes[:-1]
    big.public_witness_bytes = res.public_witness_bytes[:12] + R.to_bytes(32, "big") + res.public_witness_bytes[44:]
    short.proof_bytes = res.proof_bytes[:255]
    for each in (False, True):
        assert BW.verify_results(ctx, vk, [res, flipped, cut], each=each) == [True, False, False]
    assert BW.verify_results(ctx, vk, [cut, big, short, res]) == [False, False, False, True]
    assert BW.verify_results(ctx, vk, [cut, short]) == [False, False] and BW.verify_results(ctx, vk, []) == []
    vk.close()
    w.close()
    O.lib().oracle_pk_free(opk)
