"""Batched Groth16 verification on the GPU (zkmi_groth16_verify_many,
gpu.groth16_verify_many, Groth16Prover.verify_many): every verdict must equal
zkmi_groth16_verify's on the same proof.  Proofs: square_circuit(x) for
distinct x under one oracle key, proved on the GPU, and the reference's golden
proof under its own key.  Batch sizes sit around the 64-lane block of
k_verify_prepare / k_miller (one below, at, one above, more than two blocks)."""
import gc

import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_groth16 import _setup
from zelana_amd.r1cs import square_circuit

pytestmark = pytest.mark.gpu

Q, R = O.Q, O.R
BLOCK = 64  # lanes per block of both kernels (pairing.hip VB)
NMAX = 2 * BLOCK + 3


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def env(ctx):
    """one key, NMAX valid proofs of distinct statements (+ one more of statement 0), the resident key"""
    from zelana_amd import gpu
    cs, _ = square_circuit(2)
    opk, pkb, _, keep = _setup(cs, 91)
    pk = gpu.ProvingKey(ctx, pkb)
    vkb = pk.vk_bytes()
    rng = np.random.default_rng(5)

    def prove(x):
        _, z = square_circuit(x)
        zz = np.array([O.int_to_limbs(v) for v in z], np.uint64)
        r, s = (int.from_bytes(rng.bytes(31), "little") for _ in range(2))
        return gpu.groth16_prove(ctx, pk, cs, zz, r, s)

    xs = [2 + i for i in range(NMAX)]
    proofs = [prove(x) for x in xs]
    e = {"pk": pk, "vkb": vkb, "vk": gpu.VerifyingKey(ctx, vkb), "proofs": proofs, "inputs": [[x * x % R] for x in xs],
         "twin": prove(xs[0]), "cs": cs, "keep": keep}
    # the reference for every expected verdict: the per-proof host verifier
    assert all(gpu.groth16_verify(vkb, i, *p) for p, i in zip(proofs[:3], e["inputs"][:3]))
    return e


def host(env, proofs, inputs):
    from zelana_amd import gpu
    return [gpu.groth16_verify(env["vkb"], i, *p) for p, i in zip(proofs, inputs)]


def limbs(v):
    return np.array(O.int_to_limbs(v), np.uint64)


def neg_g1(p):
    q = np.array(p, np.uint64).copy()
    if q.any():
        q[4:] = limbs((Q - O.limbs_to_int(q[4:])) % Q)
    return q


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("nb", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, NMAX])
def test_sizes_all_valid(ctx, env, nb):
    from zelana_amd import gpu
    valid, st = gpu.groth16_verify_many(ctx, env["vk"], env["proofs"][:nb], env["inputs"][:nb])
    assert valid == [True] * nb
    if nb == 0:
        assert st == {"pairs": 0, "final_exps": 0, "invalid_points": 0}
    else:
        assert st == {"pairs": nb + 3, "final_exps": 1, "invalid_points": 0}
    if nb in (1, BLOCK + 1):  # the host loop agrees (all sizes share these proofs)
        assert host(env, env["proofs"][:nb], env["inputs"][:nb]) == valid


def test_golden_proof_under_its_key(ctx):
    from test_pairing import ref_proof, ref_vk
    from test_verify_cpu import compressed_vk
    from zelana_amd import gpu
    vkb = compressed_vk(ref_vk())
    vk = gpu.VerifyingKey(ctx, vkb)
    assert vk.n_inputs == 1
    (a, b, c), x = ref_proof()
    valid, st = gpu.groth16_verify_many(ctx, vk, [(a, b, c)] * 3, [[x], [x + 1], [x]])
    assert valid == [gpu.groth16_verify(vkb, [v], a, b, c) for v in (x, x + 1, x)] == [True, False, True]
    assert st["pairs"] == 6 and st["final_exps"] > 1
    vk.close()


# ------------------------------------------------------------------ 2. one bad proof
def fq2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def fq2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = fq2_mul(r, a)
        a = fq2_mul(a, a)
        e >>= 1
    return r


def fq2_sqrt(a):
    """q = 3 mod 4 (Adj & Rodriguez-Henriquez, Algorithm 9); None for a non-square"""
    a1 = fq2_pow(a, (Q - 3) // 4)
    alpha = fq2_mul(fq2_mul(a1, a1), a)
    x0 = fq2_mul(a1, a)
    if alpha == (Q - 1, 0):
        x = ((-x0[1]) % Q, x0[0])
    else:
        x = fq2_mul(fq2_pow(((1 + alpha[0]) % Q, alpha[1]), (Q - 1) // 2), x0)
    return x if fq2_mul(x, x) == a else None


def twist_point_outside_subgroup():
    """the first small x = k + u for which x^3 + b' is a square: a point of
    the twist, whose cofactor is ~2^254, so it is outside the order-r subgroup"""
    inv82 = pow(82, Q - 2, Q)
    bt = (27 * inv82 % Q, (-3 * inv82) % Q)  # 3 / (9 + u)
    for k in range(1, 100):
        x = (k, 1)
        x3 = fq2_mul(fq2_mul(x, x), x)
        y = fq2_sqrt(((x3[0] + bt[0]) % Q, (x3[1] + bt[1]) % Q))
        if y is not None:
            return np.concatenate([limbs(x[0]), limbs(x[1]), limbs(y[0]), limbs(y[1])])
    raise AssertionError("no twist point found")


KINDS = ["a_doubled", "c_swapped", "input_changed", "a_off_curve", "coordinate_plus_q", "b_outside_subgroup",
         "a_infinity", "b_infinity"]


@pytest.mark.parametrize("kind", KINDS)
def test_one_bad_proof(ctx, env, kind):
    from zelana_amd import gpu
    nb = BLOCK + 1
    for pos in (0, nb // 2, nb - 1):
        proofs = [tuple(np.array(v, np.uint64).copy() for v in p) for p in env["proofs"][:nb]]
        inputs = [list(i) for i in env["inputs"][:nb]]
        a, b, c = proofs[pos]
        touched = [pos]
        if kind == "a_doubled":
            proofs[pos] = (gpu.g1_add(a, a), b, c)
        elif kind == "c_swapped":
            other = (pos + 1) % nb
            proofs[pos], proofs[other] = (a, b, proofs[other][2]), (proofs[other][0], proofs[other][1], c)
            touched.append(other)
        elif kind == "input_changed":
            inputs[pos] = [(inputs[pos][0] + 1) % R]
        elif kind == "a_off_curve":
            a[4] ^= np.uint64(1)
        elif kind == "coordinate_plus_q":
            a[:4] = limbs(O.limbs_to_int(a[:4]) + Q)
        elif kind == "b_outside_subgroup":
            proofs[pos] = (a, twist_point_outside_subgroup(), c)
        elif kind == "a_infinity":
            proofs[pos] = (np.zeros(8, np.uint64), b, c)
        elif kind == "b_infinity":
            proofs[pos] = (a, np.zeros(16, np.uint64), c)
        want = [True] * nb
        for t in touched:  # the expected verdict is the host verifier's
            want[t] = gpu.groth16_verify(env["vkb"], inputs[t], *proofs[t])
            if "infinity" not in kind:  # there the verdict is whatever the host verifier says
                assert want[t] is False, (kind, t)
        valid, st = gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs)
        assert valid == want, (kind, pos)
        flagged = kind in ("a_off_curve", "coordinate_plus_q", "b_outside_subgroup")
        assert st["invalid_points"] == (1 if flagged else 0), (kind, st)
        # a proof dropped by point validation leaves a batch that passes at once; any other failure bisects
        assert (st["final_exps"] == 1) == (flagged or all(want)), (kind, st)


# ------------------------------------------------------------------ 3. weights are used
def test_weights_are_used(ctx, env):
    from zelana_amd import gpu
    (a1, b1, c1), (a2, b2, c2) = env["proofs"][0], env["twin"]  # two proofs of one statement
    d = O.gen_points_g1(321, 1)[0]
    p1, p2 = (a1, b1, gpu.g1_add(c1, d)), (a2, b2, gpu.g1_add(c2, neg_g1(d)))
    inputs = [env["inputs"][0], env["inputs"][0]]
    assert host(env, [p1, p2], inputs) == [False, False]  # each is invalid on its own
    # with equal weights the two errors cancel in the combined check (why caller-chosen weights are for tests)
    assert gpu.groth16_verify_many(ctx, env["vk"], [p1, p2], inputs, rho=[1, 1])[0] == [True, True]
    assert gpu.groth16_verify_many(ctx, env["vk"], [p1, p2], inputs)[0] == [False, False]
    assert gpu.groth16_verify_many(ctx, env["vk"], [p1, p2], inputs, rho=[3, 2**127 + 5])[0] == [False, False]


# ------------------------------------------------------------------ 4. rho handling
def test_rho_and_argument_handling(ctx, env):
    from zelana_amd import ZkmiError, gpu
    nb = 5
    proofs = [tuple(np.array(v, np.uint64).copy() for v in p) for p in env["proofs"][:nb]]
    inputs = [list(i) for i in env["inputs"][:nb]]
    inputs[3] = [inputs[3][0] + 1]
    rho = [7, 2**128 - 1, 2**64, 12345678901234567890123, 1]
    r1 = gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs, rho=rho)
    r2 = gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs, rho=rho)
    assert r1 == r2 and r1[0] == host(env, proofs, inputs) == [True, True, True, False, True]
    with pytest.raises(ZkmiError):
        gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs, rho=[7, 0, 1, 1, 1])
    inputs[1] = [R]
    with pytest.raises(ZkmiError):
        gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs)
    bad = bytearray(env["vkb"])
    bad[40] ^= 0x5A  # beta's x no longer decodes to a subgroup point
    with pytest.raises(ZkmiError):
        gpu.VerifyingKey(ctx, bytes(bad))


# ------------------------------------------------------------------ 5. Python surface
def test_prover_verify_many(ctx, env):
    from zelana_amd import gpu
    from zelana_amd.prover import BatchProof, BatchPublicInputs, Groth16Prover
    prover = Groth16Prover(ctx, env["pk"], env["vkb"], circuit=lambda i, w: None)
    bps, ins = [], []
    for k in range(6):
        a, b, c = env["proofs"][k]
        if k == 2:
            c = gpu.g1_add(c, c)
        raw = gpu.proof_to_solana_bytes(a, b, c)
        bps.append(BatchProof(BatchPublicInputs(batch_id=k), raw, 0) if k in (1, 2) else
                   BatchProof(BatchPublicInputs(batch_id=k), raw, 0, a, b, c))
        ins.append([env["inputs"][k][0] + (1 if k == 4 else 0)])
    want = [prover.verify_pairing(p, x) for p, x in zip(bps, ins)]
    assert want == [True, True, False, True, False, True]
    assert prover.verify_many(bps, ins) == want
    assert prover.verify_many([], []) == []


# ------------------------------------------------------------------ 6. lifetime
def test_key_outliving_its_context(env):
    from zelana_amd import gpu
    c2 = gpu.Context(0)
    vk = gpu.VerifyingKey(c2, env["vkb"])
    assert gpu.groth16_verify_many(c2, vk, env["proofs"][:2], env["inputs"][:2])[0] == [True, True]
    c2.close()  # frees the key first (Context._track)
    assert not vk.h
    del vk
    gc.collect()
