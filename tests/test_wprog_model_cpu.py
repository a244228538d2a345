"""tests/wprog_model.py pinned on the CPU: on small recorded programs the one
integer model of all ten op kinds must equal, bit for bit, each interpreter a
recorder ships with and the synthesised assignment z.  The GPU comparison
(test_gpu_wprog_ops.py) rests on this.

  kinds 1-4   zelana_batch, reduced shapes   wprog.Plan.interpret
  kinds 1, 5-8  L2BlockCircuit               host_prover.L2Program.interpret (C++)
  kinds 9, 10  ShieldedTransferCircuit       shielded.interpret
"""
import numpy as np
import pytest

import wprog_model as M
from test_l2_wprog import SHAPES, _batch
from test_shielded_cpu import _notes


def _same(got, want):
    bad = np.nonzero((got != want).any(1))[0]
    assert got.shape == want.shape and bad.size == 0, f"z differs at {bad[:8]} of {want.shape[0]}"


@pytest.mark.parametrize("depth,ntx", [(2, 1), (3, 2)])
def test_model_equals_plan_interpret(depth, ntx):
    from zelana_amd import wprog as W, zbatch as Z
    kw = dict(max_transfers=ntx, max_withdrawals=1, max_shielded=1, depth=depth)
    d = Z.synthetic_batch(depth, ntx, seed=100 + depth)
    plan, _, z = W.record(d, **kw)
    assert set(plan.kinds.tolist()) == {M.MUL, M.INV, M.BITS64, M.PERM}
    inp = Z.batch_inputs(d, **kw)
    got = M.limbs(M.interpret(plan, inp))
    _same(got, z)
    _same(got, plan.interpret(inp))
    d2 = Z.synthetic_batch(depth, ntx, seed=7 + depth)
    inp2 = Z.batch_inputs(d2, **kw)
    _, z2, _ = Z.build(d2, witness_only=True, **kw)
    got2 = M.limbs(M.interpret(plan, inp2))
    _same(got2, z2)
    _same(got2, plan.interpret(inp2))


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_model_equals_l2_interpret(shape):
    from zelana_amd import host_prover as H
    bal, tr, wd = SHAPES[shape]
    inp, w = _batch(5, bal, tr, wd)
    _, z, prog = H.l2_record(inp, w)
    assert set(prog.kinds.tolist()) == {M.MUL, M.BITS, M.NZ, M.POSEIDON, M.INV1}
    got = M.limbs(M.interpret(prog, prog.template_inputs))
    _same(got, z)
    _same(got, prog.interpret(prog.template_inputs))
    # other values of the shape, one balance overdrawn (an inconsistent batch is proved too)
    inp2, w2 = _batch(2 ** 63, {k: v * 1000 + 3 for k, v in bal.items()}, [(a, b, amt * 1000 + 1) for a, b, amt in tr],
                      tuple((b, amt + 1000) for b, amt in wd), 200)
    x2 = H.l2_witness_inputs(inp2, w2)
    _, z2 = H.native_l2_block_circuit(inp2, w2)
    got2 = M.limbs(M.interpret(prog, x2))
    _same(got2, z2)
    _same(got2, prog.interpret(x2))


def test_model_equals_shielded_interpret():
    from zelana_amd import shielded as S
    ts = [_notes(2, 1, 1, salt=s) for s in (0, 4)]
    ts[1].fee += 1  # unsatisfied: the program still computes the synthesis z
    _, z0, prog, _ = S.record(ts[0])
    assert set(prog.kinds.tolist()) == {M.POSEIDON_RC, M.SELECT}
    for t, z in ((ts[0], z0), (ts[1], S.synthesize(ts[1])[1])):
        x = S.witness_inputs(t)
        got = M.interpret(prog, x)
        assert got == [int(v) for v in z]
        assert got == S.interpret(prog, x)


def test_builder_layout_and_levels():
    """the builder's arrays against a program written out by hand"""
    # inputs 0 (One), 1, 2; MUL -> 3; BITS(3) of it -> 4..6; NZ pushed to level 4 -> 7
    ops = [(M.MUL, 3, 0, [[(1, 1), (0, M.R - 1)], [(2, 5)]]),
           (M.BITS, 4, 3, [[(3, 1)]]),
           (M.NZ, 7, 0, [[]], 4)]
    p = M.build(8, [0, 1, 2], ops)
    assert p.level_start.tolist() == [0, 1, 2, 2, 3] and p.level_sizes() == [1, 1, 0, 1]
    assert p.op.tolist() == [[1 | (2 << 8) | (1 << 20), 3, 0, 2], [5 | (1 << 8), 4, 3, 3], [6, 7, 4, 0]]
    assert p.term.tolist() == [[1, 0], [0, 1], [2, 2], [3, 0]]
    assert M._ints(p.coeff) == [1, M.R - 1, 5]
    z = M.interpret(p, M.limbs([1, 7, 3]))
    assert z == [1, 7, 3, 18 * 5 % M.R, 0, 1, 0, 0]
    # permutations lead their level unless the caller's order is kept
    ops = [(M.MUL, 2, 0, [[(1, 1)], [(1, 1)]]), (M.PERM, 3, 0, [[(1, 1)]])]
    assert M.build(367, [0, 1], ops).kinds.tolist() == [M.PERM, M.MUL]
    assert M.build(367, [0, 1], ops, keep_order=True).kinds.tolist() == [M.MUL, M.PERM]
    with pytest.raises(AssertionError):  # a permutation's inner trace values are not readable
        M.build(368, [0, 1], ops + [(M.NZ, 367, 0, [[(3, 1)]])])
    with pytest.raises(AssertionError):  # an override may not lift an op above what it reads
        M.build(368, [0, 1], ops + [(M.NZ, 367, 0, [[(366, 1)]], 1)])


def test_gpu_operand_set_is_what_it_claims():
    """the operand set of test_gpu_wprog_ops.py: every combination equals its
    slot mod r (and is not the slot's single term), the zero forms are 0, in
    every batch; the edge values and combination lengths are all there"""
    import test_gpu_wprog_ops as G
    for seed in range(1, 7):
        E = G.Operands(seed)
        for x in E.inputs():
            z = M._ints(x)
            assert z[:3] == [1, 0, 1] and set(G.EDGE) <= set(z)

            def ev(lc):
                return sum(z[v] * c for v, c in lc) % M.R
            assert all(ev(lc) == 0 for _, lc in E.zeros)
            assert all(ev(s[1]) == ev(m[1]) == z[v] and len(m[1]) >= 3
                       for s, m, v in zip(E.single, E.multi, E.slot))
        assert {len(lc) for _, lc in E.all} == {0, 1, 2, 3, 4, 5, 8, 9}
        assert {0, 1, M.R - 1} <= {c for _, lc in E.all for _, c in lc}
        # the 8-term zero: a running total that passes r several times (batch 0)
        z = M._ints(E.inputs()[0])
        assert sum(z[v] * c % M.R for v, c in E.zeros[5][1]) >= 2 * M.R
    assert {M.R - 1, M.R - 2, (M.R - 1) // 2, (M.R + 1) // 2, 2 ** 29 - 1, 2 ** 29, 2 ** 58, 2 ** 64 - 1, 2 ** 64,
            2 ** 232, 2 ** 253} <= set(G.EDGE)
    for k in (1, 2, 4, 8):  # all-ones low limbs, and the next such value is past r
        t = G._top(k)
        assert t < M.R <= t + (1 << (29 * k)) and t % (1 << (29 * k)) == (1 << (29 * k)) - 1


def test_mimc_model_known_answer():
    """the PERM trace's output against x -> (x + c_i)^7 iterated, with zbatch's constants"""
    from zelana_amd import zbatch as Z
    assert M.MIMC_C == [int(c) for c in Z.RC] and M.R == Z.R
    p = M.build(2 + 364, [0, 1], [(M.PERM, 2, 0, [[(1, 1)]])])
    for x in (0, 1, M.R - 2, M.R - 1, 1 << 253):
        z = M.interpret(p, M.limbs([1, x]))
        assert z[-1] == _perm_out(x) and z[2] == pow(x + 2, 2, M.R)


def _perm_out(x):
    for c in M.MIMC_C:
        x = pow((x + c) % M.R, 7, M.R)
    return x
