"""ShieldedTransferCircuit on the GPU: the two witness-program kinds it needs
(wprog.hip POSEIDON_RC, kind 9, and SELECT, kind 10) against the plain-integer
interpreter, zkmi_wprog_create's rejections, the recorded program against the
host synthesis, and ShieldedProver's batched proofs against the oracle's on the
same matrices, z, r, s, with the batched verifiers over them.

Every program runs twice: as the library schedules it (runs of small
POSEIDON_RC / SELECT levels in one k_wprog_chain launch) and with one launch
per level (ZKMI_DEBUG_WPROG_NO_RC_CHAIN=1, read by zkmi_wprog_create).
"""
import copy
import ctypes
import os

import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_groth16 import _oracle_prove, _setup
from test_shielded_cpu import _notes, _tampered

pytestmark = pytest.mark.gpu

R = O.R
EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


def _programs(ctx, prog):
    """the program as scheduled by default and with per-level launches only"""
    from zelana_amd import wprog as W
    out = [W.WitnessProgram(ctx, prog)]
    os.environ["ZKMI_DEBUG_WPROG_NO_RC_CHAIN"] = "1"
    try:
        out.append(W.WitnessProgram(ctx, prog))
    finally:
        del os.environ["ZKMI_DEBUG_WPROG_NO_RC_CHAIN"]
    return out


def _check_runs(ctx, prog, input_sets, nb_many):
    """run on input_sets[0] and run_many on the first nb_many sets (padded stride) == interpret"""
    from zelana_amd import gpu, shielded as S
    nv = prog.num_vars
    want = [S.z_limbs(S.interpret(prog, x)) for x in input_sets[:nb_many]]
    stride = nv * 32 + 96
    for wp in _programs(ctx, prog):
        dz = gpu.DeviceBuffer(ctx, nb_many * stride)
        try:
            wp.run(input_sets[0], dz)
            got = dz.download(np.zeros((nv, 4), np.uint64))
            bad = np.nonzero((got != want[0]).any(1))[0]
            assert bad.size == 0, f"run: z differs at {bad[:8]} of {nv}"
            dz.upload(np.full(nb_many * stride // 8, 0xA5A5A5A5A5A5A5A5, np.uint64))
            wp.run_many(input_sets[:nb_many], dz, stride)
            raw = dz.download(np.zeros((nb_many, stride // 8), np.uint64))
            for i in range(nb_many):
                got = raw[i, :nv * 4].reshape(nv, 4)
                bad = np.nonzero((got != want[i]).any(1))[0]
                assert bad.size == 0, f"run_many batch {i}: z differs at {bad[:8]} of {nv}"
                assert (raw[i, nv * 4:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), "pad bytes written"
        finally:
            wp.close()
            dz.free()


# ------------------------------------------------------- 1. hand-built program
NIN = 12  # One, then 11 free values


def _hand_program():
    """Level 1: 65 independent POSEIDON_RC ops (two 256-thread blocks), masks 1..7
    cycling; level 2: 65 SELECTs over their outputs with conditions 0, 1 and a
    non-bit value; level 3: two permutations and a SELECT reading level 2."""
    from zelana_amd import shielded as S
    rng = np.random.default_rng(11)

    def c():
        return int.from_bytes(rng.bytes(32), "little") % R

    def lc(nvar, const=True):  # a combination of nvar inputs (and One)
        terms = [(int(v), c()) for v in rng.choice(np.arange(1, NIN), nvar, replace=False)]
        return terms + ([(0, c())] if const else [])

    ops, at, outs = [], NIN, []
    for i in range(65):
        mask = 1 + i % 7
        lcs = [lc(1 + (i + q) % 5) if (mask >> q) & 1 else ([(0, c())] if (i + q) % 3 else []) for q in range(3)]
        ops.append((S.KIND_POSEIDON_RC, at, mask, lcs))
        span = S.permutation_rows(mask)
        outs.append(at + span - 9 + 3 * (i % 3) + 2)  # one of the last round's x^5
        at += span
    sel_out = []
    for i in range(65):
        cond = [[(1, 1)], [(2, 1)], [(3, 1)], [(1, 1), (2, 1), (0, R - 1)], lc(2)][i % 5]  # 0, 1, non-bit, 0, random
        t_lc, f_lc = [(outs[i], c()), (4, 1)], [(outs[(i + 1) % 65], 1)] + lc(i % 3, False)
        ops.append((S.KIND_SELECT, at, 0, [cond, t_lc, f_lc]))
        sel_out.append(at)
        at += 1
    for i, mask in enumerate((7, 5)):
        lcs = [[(sel_out[3 * i + q], c()), (sel_out[40 + q], 1)] if (mask >> q) & 1 else [(0, c())] for q in range(3)]
        ops.append((S.KIND_POSEIDON_RC, at, mask, lcs))
        at += S.permutation_rows(mask)
    ops.append((S.KIND_SELECT, at, 0, [[(sel_out[7], 1)], [(sel_out[8], 1)], [(sel_out[9], 2)]]))
    at += 1
    prog = S.build_program(at, 1, np.arange(NIN, dtype=np.uint32), ops)
    assert list(np.diff(prog.level_start.astype(np.int64))) == [65, 65, 3]
    inputs = []
    for k in range(3):
        vals = [1, 0, 1, 5 + k] + [c() for _ in range(NIN - 4)]
        inputs.append(S.z_limbs(vals))
    return prog, inputs


def test_hand_built_program(ctx):
    prog, inputs = _hand_program()
    _check_runs(ctx, prog, inputs, 3)


# ----------------------------------------------------------- 2. rejections
def _create(ctx, p):
    from zelana_amd._lib import WprogDesc, lib, vp
    d = WprogDesc()
    d.num_vars, d.num_inputs, d.input_var = p["num_vars"], p["input_var"].size, p["input_var"].ctypes.data
    d.num_ops, d.op = p["op"].shape[0], p["op"].ctypes.data
    d.num_terms, d.term = p["term"].shape[0], p["term"].ctypes.data
    d.num_coeffs, d.coeff = p["coeff"].shape[0], p["coeff"].ctypes.data
    d.num_levels, d.level_start = p["level_start"].size - 1, p["level_start"].ctypes.data
    h = vp()
    rc = lib().zkmi_wprog_create(ctx.h, ctypes.byref(d), ctypes.byref(h))
    if rc == 0:
        lib().zkmi_wprog_destroy(h)
    return rc


def _small():
    """two POSEIDON_RC ops (8 + 57 rounds, masks 7 and 3), then a SELECT; exactly 204 coefficients"""
    from zelana_amd import shielded as S
    w7, w3 = S.pack_pos_word(1, 7, 8, 57), S.pack_pos_word(0, 3, 8, 57)
    term = np.array([[1, 0], [2, 1], [3, 2], [1, 3], [2, 4], [1, 0], [2, 0], [3, 0]], np.uint32)
    n7, n3 = 243, 240
    op = np.array([[9 | (1 << 8) | (1 << 20), 4, 0, w7], [9 | (1 << 8) | (1 << 20), 4 + n7, 3, w3],
                   [10 | (1 << 8) | (1 << 20), 4 + n7 + n3, 5, 1]], np.uint32)
    coeff = np.zeros((204, 4), np.uint64)
    coeff[:, 0] = np.arange(1, 205)
    return dict(num_vars=4 + n7 + n3 + 1, input_var=np.arange(4, dtype=np.uint32), op=op, term=term, coeff=coeff,
                level_start=np.array([0, 2, 3], np.uint32))


def _mut(**kw):
    p = _small()
    for k, v in kw.items():
        if callable(v):
            v(p)
        else:
            p[k] = v
    return p


def _setw3(i, w):
    def f(p):
        p["op"][i, 3] = w
    return f


def test_wprog_create_rejections(ctx):
    from zelana_amd import shielded as S
    assert _create(ctx, _small()) == 0
    pw = S.pack_pos_word
    l2_pos = np.array([7 | (1 << 8) | (1 << 20), 4 + 243, 3, 0 | (3 << 16)], np.uint32)  # a kind-7 op, mask 3

    def kind(i, k):
        def f(p):
            p["op"][i, 0] = (p["op"][i, 0] & ~np.uint32(0xFF)) | np.uint32(k)
        return f

    def l2(p):
        p["op"][1] = l2_pos

    def a_off(i, v):
        def f(p):
            p["op"][i, 2] = v
        return f

    def big_coeff(p):
        p["coeff"] = np.concatenate([p["coeff"], p["coeff"]])

    def l2_first(p):
        p["op"][0] = np.array([7 | (1 << 8) | (1 << 20), 4, 0, 1 | (7 << 16)], np.uint32)

    def rounds(rp):  # both permutations with 8 + rp rounds, in a z wide enough for their traces
        return _mut(c=big_coeff, num_vars=2000, a=_setw3(0, pw(1, 7, 8, rp)), b=_setw3(1, pw(0, 3, 8, rp)))

    assert _create(ctx, rounds(64)) == 0  # 72 rounds: what the LDS table holds
    assert _create(ctx, _mut(a=l2, b=l2_first)) == 0  # kind 7 alone (with a SELECT)
    cases = {
        "mask 0": _mut(a=_setw3(0, pw(1, 0, 8, 57))),
        "R_f/2 = 0": _mut(a=_setw3(0, pw(1, 7, 0, 57))),
        "rounds beyond the LDS table": rounds(65),
        "two round settings": _mut(c=big_coeff, b=_setw3(1, pw(0, 3, 8, 56))),
        "kinds 7 and 9": _mut(a=l2),
        "num_coeffs below 3 (R_f + R_p) + 9": _mut(coeff=_small()["coeff"][:203]),
        "trace past num_vars": _mut(num_vars=_small()["num_vars"] - 2, level_start=np.array([0, 2, 2], np.uint32),
                                    op=_small()["op"][:2]),
        "POSEIDON_RC terms past num_terms": _mut(a=a_off(0, 6)),
        "SELECT terms past num_terms": _mut(a=a_off(2, 6)),
        "SELECT with high bits in word 3": _mut(a=_setw3(2, 1 | (1 << 16))),
        "SELECT out past num_vars": _mut(num_vars=_small()["num_vars"] - 1),
        "unknown kind 11": _mut(a=kind(2, 11)),
    }
    # (the shortened program of "trace past num_vars" is accepted with its full num_vars)
    assert _create(ctx, _mut(level_start=np.array([0, 2, 2], np.uint32), op=_small()["op"][:2])) == 0
    assert _create(ctx, _mut(c=big_coeff)) == 0
    for name, p in cases.items():
        assert _create(ctx, p) == EINVAL, name
    # reading a trace value other than the last round's x^5 is refused for kind 9 as for kind 7
    bad = _small()
    bad["term"][5, 0] = 4 + 243 - 9  # the last round's first x^2
    assert _create(ctx, bad) == EINVAL
    ok = _small()
    ok["term"][5, 0] = 4 + 243 - 9 + 2
    assert _create(ctx, ok) == 0


def test_kind7_program_still_accepted(ctx):
    from test_l2_wprog import SHAPES, _batch
    from zelana_amd import host_prover as H, wprog as W
    _, _, plan = H.l2_record(*_batch(5, *SHAPES[0]))
    assert (plan.kinds == 7).any()
    W.WitnessProgram(ctx, plan).close()


# ------------------------------------------------ 3. the recorded program
@pytest.mark.parametrize("depth,n_in,n_out", [(2, 1, 1), (3, 2, 2)])
def test_shielded_program_equals_synthesis(ctx, depth, n_in, n_out):
    from zelana_amd import shielded as S
    honest = [_notes(depth, n_in, n_out, salt=s) for s in (0, 4, 8)]
    if n_in == 2:
        bad = [_tampered(honest[0], "sibling")[0], _tampered(honest[1], "spending_key")[0]]
    else:
        bad = [copy.deepcopy(honest[0]), copy.deepcopy(honest[1])]
        bad[0].inputs[0].merkle_path[1] = bytes([7] * 32)
        bad[1].fee += 1
    ts = [honest[0], bad[0], honest[1], bad[1], honest[2]]
    _, z0, prog, _ = S.record(ts[0])
    zs = [z0] + [S.synthesize(t)[1] for t in ts[1:]]
    inputs = [S.witness_inputs(t) for t in ts]
    for x, z in zip(inputs, zs):  # the interpreter is the reference of _check_runs: it gives the synthesis z
        assert S.interpret(prog, x) == z
    _check_runs(ctx, prog, inputs, 5)


# ------------------------------------------------------------- 4. proofs
def test_prove_many_matches_oracle_and_verifies(ctx):
    from zelana_amd import gpu, shielded as S
    from zelana_amd.rng import StdRng
    ts = [_notes(3, 2, 2, salt=s) for s in (0, 1, 2, 3)]
    bad, name, k = _tampered(_notes(3, 2, 2, salt=6), "path_bit")
    ts.insert(2, bad)
    seeds = [5, 6, 7, 8, 2 ** 40]
    sp = S.ShieldedProver(ctx, (3, 3, 2), seed=3, check=True)
    opk, _, _, (st, keep) = _setup(sp.r1cs, 3)
    try:
        proofs = sp.prove_many(ts, seeds)
        for i, (t, p) in enumerate(zip(ts, proofs)):
            cs, z, eq = S.synthesize(t)
            assert cs.rows == sp.r1cs.rows
            rng = StdRng.seed_from_u64(seeds[i])
            r, s = rng.fr_rand(), rng.fr_rand()
            a, b, c = _oracle_prove(opk, st, S.z_limbs(z), r, s)
            assert np.array_equal(p.a, a) and np.array_equal(p.b, b) and np.array_equal(p.c, c), i
            assert p.public_inputs == S.public_inputs_fr(t)
            first = S.first_unsatisfied(cs, z)
            assert (first == eq[name][k]) if i == 2 else first is None
            assert p.constraints_ok == (i != 2) and p.first_unsatisfied == first
            ok = gpu.groth16_verify(sp.verifying_key, p.public_inputs, p.a, p.b, p.c)
            assert ok == (i != 2)
        want = [i != 2 for i in range(5)]
        assert sp.verify_many(proofs) == want
        assert sp.verify_each(proofs) == want
        # without the check the statuses stay None and the proofs are the same
        sp.check = False
        again = sp.prove_many(ts[:2], seeds[:2])
        assert all(q.constraints_ok is None and q.first_unsatisfied is None for q in again)
        assert all(np.array_equal(q.a, p.a) and np.array_equal(q.c, p.c) for q, p in zip(again, proofs))
    finally:
        O.lib().oracle_pk_free(opk)
        sp.close()


# ----------------------------------------------------- 5. the real shape
def test_real_shape_end_to_end(ctx):
    """(2,2) depth 32: keygen, prove_many at nb = 4, verify_many_encoded from compressed bytes"""
    from zelana_amd import gpu, shielded as S
    ts = [_notes(32, 2, 2, salt=s) for s in range(4)]
    sp = S.ShieldedProver(ctx, (32, 32, 2), seed=0)
    try:
        assert sp.r1cs.num_constraints == 18927 and sp.pk.n == 1 << 15
        proofs = sp.prove_many(ts, [100, 101, 102, 103])
        raws = [p.compressed() for p in proofs]
        assert all(len(r) == 128 for r in raws)
        pubs = [p.public_inputs for p in proofs]
        assert sp.verify_many_encoded(gpu.PROOF_ARK_COMPRESSED, raws, pubs) == [True] * 4
        assert sp.verify_many_encoded(gpu.PROOF_ARK_COMPRESSED, b"".join(raws), pubs, each=True) == [True] * 4
        pubs[1] = pubs[1][:-1] + [(pubs[1][-1] + 1) % R]  # another fee
        assert sp.verify_many_encoded(gpu.PROOF_ARK_COMPRESSED, raws, pubs) == [True, False, True, True]
        assert sp.verify_many_encoded(gpu.PROOF_ARK_COMPRESSED, raws, pubs, each=True) == [True, False, True, True]
    finally:
        sp.close()
