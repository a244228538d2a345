"""Exact per-proof Groth16 verdicts from the GPU (zkmi_groth16_verify_each,
gpu.groth16_verify_each, Groth16Prover.verify_each) and the probe budget of
verify_many (Context.set_verify_probes, gpu.groth16_verify_last): every verdict
must equal zkmi_groth16_verify's on the same proof.  Proofs as
test_gpu_verify_many's: square_circuit(x) for distinct x under one oracle key,
the reference's golden proof under its own key, and synthetic(8, 8, 16) for
seven public inputs.  Sizes: 3 * 21 + 1 = 64 pairs fill exactly one block of
k_miller and 22 is the first size past it; 63 / 64 / 65 straddle the block of
the per-proof kernels; 131 spans more than two."""
import gc

import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_groth16 import _setup
from test_gpu_verify_many import (BLOCK, KINDS, NMAX, ctx, env, host, limbs, neg_g1,  # noqa: F401 (fixtures)
                                  twist_point_outside_subgroup)

pytestmark = pytest.mark.gpu

Q, R = O.Q, O.R
NB = BLOCK + 1


def each_stats(nb, flagged=0):
    if nb == flagged:
        return {"pairs": 0, "final_exps": 0, "invalid_points": flagged}
    return {"pairs": 3 * nb + 1, "final_exps": nb - flagged, "invalid_points": flagged}


def copies(env, nb):
    return ([tuple(np.array(v, np.uint64).copy() for v in p) for p in env["proofs"][:nb]],
            [list(i) for i in env["inputs"][:nb]])


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("nb", [0, 1, 21, 22, BLOCK - 1, BLOCK, BLOCK + 1, NMAX])
def test_each_sizes_all_valid(ctx, env, nb):
    from zelana_amd import gpu
    assert NMAX == 131
    valid, st = gpu.groth16_verify_each(ctx, env["vk"], env["proofs"][:nb], env["inputs"][:nb])
    assert valid == [True] * nb
    assert st == each_stats(nb)
    if nb in (1, BLOCK + 1):
        assert host(env, env["proofs"][:nb], env["inputs"][:nb]) == valid


# ------------------------------------------------------------------ 2. the eight kinds of bad proof
def tamper(kind, proofs, inputs, pos):
    """test_gpu_verify_many.test_one_bad_proof's changes; returns the touched positions"""
    from zelana_amd import gpu
    nb = len(proofs)
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
    else:
        raise AssertionError(kind)
    return touched


@pytest.mark.parametrize("kind", KINDS)
def test_each_one_bad_proof(ctx, env, kind):
    from zelana_amd import gpu
    assert len(KINDS) == 8
    for pos in (0, NB // 2, NB - 1):
        proofs, inputs = copies(env, NB)
        touched = tamper(kind, proofs, inputs, pos)
        want = [True] * NB
        for t in touched:  # the expected verdict is the host verifier's
            want[t] = gpu.groth16_verify(env["vkb"], inputs[t], *proofs[t])
            if "infinity" not in kind:
                assert want[t] is False, (kind, t)
        valid, st = gpu.groth16_verify_each(ctx, env["vk"], proofs, inputs)
        assert valid == want, (kind, pos)
        flagged = kind in ("a_off_curve", "coordinate_plus_q", "b_outside_subgroup")
        assert st == each_stats(NB, 1 if flagged else 0), (kind, st)


# ------------------------------------------------------------------ 3. all bad, mixed, every point flagged
def test_each_all_bad_and_mixed(ctx, env):
    from zelana_amd import gpu
    proofs, inputs = copies(env, NB)
    all_bad = [[(x[0] + 1) % R] for x in inputs]
    valid, st = gpu.groth16_verify_each(ctx, env["vk"], proofs, all_bad)
    assert valid == [False] * NB and st == each_stats(NB)
    mixed = [all_bad[i] if i % 2 else inputs[i] for i in range(NB)]
    valid, st = gpu.groth16_verify_each(ctx, env["vk"], proofs, mixed)
    assert valid == host(env, proofs, mixed) == [i % 2 == 0 for i in range(NB)]
    assert st == each_stats(NB)
    # nothing passes point validation: no Miller loop, no final exponentiation
    for a, _, _ in proofs[:3]:
        a[4] ^= np.uint64(1)
    valid, st = gpu.groth16_verify_each(ctx, env["vk"], proofs[:3], inputs[:3])
    assert valid == [False] * 3 and st == each_stats(3, 3)


def test_each_no_cancellation(ctx, env):
    """test_weights_are_used's two proofs (C + D, C - D): their errors cancel
    in verify_many under equal weights; verify_each has no weights"""
    from zelana_amd import gpu
    (a1, b1, c1), (a2, b2, c2) = env["proofs"][0], env["twin"]
    d = O.gen_points_g1(321, 1)[0]
    p1, p2 = (a1, b1, gpu.g1_add(c1, d)), (a2, b2, gpu.g1_add(c2, neg_g1(d)))
    inputs = [env["inputs"][0], env["inputs"][0]]
    assert gpu.groth16_verify_many(ctx, env["vk"], [p1, p2], inputs, rho=[1, 1])[0] == [True, True]
    assert gpu.groth16_verify_each(ctx, env["vk"], [p1, p2], inputs)[0] == host(env, [p1, p2], inputs) == [False, False]


def test_each_golden_proof_under_its_key(ctx):
    from test_pairing import ref_proof, ref_vk
    from test_verify_cpu import compressed_vk
    from zelana_amd import gpu
    vkb = compressed_vk(ref_vk())
    vk = gpu.VerifyingKey(ctx, vkb)
    (a, b, c), x = ref_proof()
    valid, st = gpu.groth16_verify_each(ctx, vk, [(a, b, c)] * 3, [[x], [x + 1], [x]])
    assert valid == [gpu.groth16_verify(vkb, [v], a, b, c) for v in (x, x + 1, x)] == [True, False, True]
    assert st == each_stats(3)
    vk.close()


# ------------------------------------------------------------------ 4. seven public inputs
def test_each_more_inputs(ctx):
    """synthetic(8, 8, 16): the public inputs are free variables, so one
    proof's are set to 0 and r - 1 and the product witnesses recomputed"""
    from zelana_amd import ZkmiError, gpu
    from zelana_amd.r1cs import synthetic
    cs, zarr = synthetic(8, 8, 16)
    opk, pkb, _, keep = _setup(cs, 33)
    pk = gpu.ProvingKey(ctx, pkb)
    vkb = pk.vk_bytes()
    vk = gpu.VerifyingKey(ctx, vkb)
    assert vk.n_inputs == 7
    z0 = [O.limbs_to_int(v) for v in zarr]
    nv, m = len(z0), 8

    def assignment(changes):
        z = list(z0)
        for k, v in changes.items():
            z[k] = v
        for i in range(m):  # the product witness of row i (r1cs.synthetic)
            av = sum(c * z[j] for j, c in cs.rows["a"][i]) % R
            bv = sum(c * z[j] for j, c in cs.rows["b"][i]) % R
            z[nv - m + i] = av * bv % R
        assert cs.is_satisfied(z)
        return z

    rng = np.random.default_rng(9)
    zs = [assignment({}), assignment({1: 0, 2: R - 1}), assignment({3: 12345, 7: 1})]
    proofs, inputs = [], []
    for z in zs:
        zz = np.array([O.int_to_limbs(v) for v in z], np.uint64)
        r, s = (int.from_bytes(rng.bytes(31), "little") for _ in range(2))
        proofs.append(gpu.groth16_prove(ctx, pk, cs, zz, r, s))
        inputs.append(z[1:8])

    def hostv(ins):
        return [gpu.groth16_verify(vkb, i, *p) for p, i in zip(proofs, ins)]

    valid, st = gpu.groth16_verify_each(ctx, vk, proofs, inputs)
    assert valid == hostv(inputs) == [True] * 3 and st == each_stats(3)
    for d in (1, R - 1):  # one input of each proof moved up, then down
        moved = [list(x) for x in inputs]
        for k in range(3):
            moved[k][2 * k] = (moved[k][2 * k] + d) % R
        assert gpu.groth16_verify_each(ctx, vk, proofs, moved)[0] == hostv(moved) == [False] * 3
    one = [list(x) for x in inputs]
    one[1][0] = 1  # was 0
    assert gpu.groth16_verify_each(ctx, vk, proofs, one)[0] == hostv(one) == [True, False, True]
    one[2][6] = R
    with pytest.raises(ZkmiError):
        gpu.groth16_verify_each(ctx, vk, proofs, one)
    vk.close()
    pk.close()
    O.lib().oracle_pk_free(opk)
    del keep


# ------------------------------------------------------------------ 5. the probe budget of verify_many
def test_budget_all_bad(ctx, env):
    from zelana_amd import gpu
    proofs, inputs = copies(env, NB)
    all_bad = [[(x[0] + 1) % R] for x in inputs]
    try:
        ctx.set_verify_probes(1)
        assert ctx.get_verify_probes() == 1
        valid, st = gpu.groth16_verify_many(ctx, env["vk"], proofs, all_bad)
        assert valid == [False] * NB
        assert st == {"pairs": NB + 3, "final_exps": 1, "invalid_points": 0}
        assert gpu.groth16_verify_last(ctx) == {"gpu_decided": NB, "gpu_pairs": 3 * NB + 1, "gpu_final_exps": NB}
        ctx.set_verify_probes(4)
        valid, st = gpu.groth16_verify_many(ctx, env["vk"], proofs, all_bad)
        assert valid == [False] * NB and st["final_exps"] <= 4
        last = gpu.groth16_verify_last(ctx)
        assert 0 < last["gpu_decided"] <= NB and last["gpu_final_exps"] == last["gpu_decided"]
        # a mixed batch under a small budget: the verdicts are still the host's
        mixed = [all_bad[i] if i % 2 else inputs[i] for i in range(NB)]
        valid, st = gpu.groth16_verify_many(ctx, env["vk"], proofs, mixed)
        assert valid == [i % 2 == 0 for i in range(NB)] and st["final_exps"] <= 4
    finally:
        ctx.set_verify_probes(0)


def test_budget_one_bad_and_reset(ctx, env):
    from zelana_amd import gpu
    proofs, inputs = copies(env, NB)
    inputs[NB // 2] = [(inputs[NB // 2][0] + 1) % R]
    want = [i != NB // 2 for i in range(NB)]
    free = gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs)
    assert free[0] == want
    try:
        ctx.set_verify_probes(64)
        assert gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs) == free
        assert gpu.groth16_verify_last(ctx) == {"gpu_decided": 0, "gpu_pairs": 0, "gpu_final_exps": 0}
        ctx.set_verify_probes(2)  # the budget is hit, then cleared by the next call that does not hit it
        assert gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs)[0] == want
        assert gpu.groth16_verify_last(ctx)["gpu_decided"] > 0
    finally:
        ctx.set_verify_probes(0)
    assert ctx.get_verify_probes() == 0
    # the default again: test_sizes_all_valid's stats shape
    for nb in (0, 1, NB):
        valid, st = gpu.groth16_verify_many(ctx, env["vk"], env["proofs"][:nb], env["inputs"][:nb])
        assert valid == [True] * nb
        assert st == ({"pairs": nb + 3, "final_exps": 1, "invalid_points": 0} if nb else
                      {"pairs": 0, "final_exps": 0, "invalid_points": 0})
        assert gpu.groth16_verify_last(ctx) == {"gpu_decided": 0, "gpu_pairs": 0, "gpu_final_exps": 0}
    assert gpu.groth16_verify_many(ctx, env["vk"], proofs, inputs) == free


# ------------------------------------------------------------------ 6. Python surface, lifetime
def test_prover_verify_each(ctx, env):
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
    assert prover.verify_each(bps, ins) == want
    assert prover.verify_each([], []) == []


def test_each_key_of_another_context_and_lifetime(ctx, env):
    from zelana_amd import ZkmiError, gpu
    c2 = gpu.Context(0)
    vk = gpu.VerifyingKey(c2, env["vkb"])
    assert gpu.groth16_verify_each(c2, vk, env["proofs"][:2], env["inputs"][:2])[0] == [True, True]
    with pytest.raises(ZkmiError):
        gpu.groth16_verify_each(ctx, vk, env["proofs"][:2], env["inputs"][:2])
    c2.close()  # frees the key first (Context._track)
    assert not vk.h
    del vk
    gc.collect()
