"""wprog.hip's ten op kinds against the plain-integer model (wprog_model.py) at
the operands and level shapes where its private arithmetic and its scheduler
can go wrong and no recorded program goes.

The kernels use lazily reduced 9 x 29-bit Montgomery routines of their own
(mul_ilp, sqr_ilp, mul3_ilp, redc_fr, pow_w3) whose "< 2p" arguments live in
comments, so every kind is fed the operand set E below, each value both as one
input with coefficient 1 and as combinations that equal it only mod r (lengths
0, 1, 3, 4, 5, 8, 9: eval_lc unrolls by four; coefficients 0, 1, r - 1 among
them).  zkmi_wprog_run_many picks one of five kernel instances per level, so
the geometry programs pin its boundaries (64 ops a block, 256 ops a chainable
level, runs of 1 / 2 / 3 levels, empty levels) and the order programs the
kinds that must not be judged by a level's first op.

Every comparison is np.array_equal on canonical limbs over the whole z.  The
buffer (three strides, padding included) is filled with 0xA5A5... before each
run, so an op that writes nothing shows, and everything outside the z of the
batches run must still hold the filler afterwards.  Every program goes through
run and through run_many with 1, 2 and 3 batches of different inputs.
"""
import os

import numpy as np
import pytest

import wprog_model as M
from wprog_model import BITS, BITS64, INV, INV1, MUL, NZ, PERM, POSEIDON, POSEIDON_RC, R, SELECT

pytestmark = pytest.mark.gpu

SENT = np.uint64(0xA5A5A5A5A5A5A5A5)
NB = 3
ONE, ZERO, UNIT = 0, 1, 2  # inputs every program here starts with: One, a 0 and a 1


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ running
def _open(ctx, prog, env=None):
    """the program on the GPU, or None when zkmi_wprog_create refuses it with ZKMI_EINVAL"""
    from zelana_amd import wprog as W
    from zelana_amd._lib import ZkmiError
    if env:
        os.environ[env] = "1"
    try:
        return W.WitnessProgram(ctx, prog)
    except ZkmiError as e:
        if "failed (-1)" in str(e):
            return None
        raise
    finally:
        if env:
            del os.environ[env]


def _what(prog, var):
    for i, (w0, out, _, w3) in enumerate(prog.op.tolist()):
        if out <= var < out + M.span(w0 & 0xFF, w3):
            lv = int(np.searchsorted(prog.level_start, i, side="right")) - 1
            return f"z[{var}] = value {var - out} of op {i} (kind {w0 & 0xFF}, level {lv})"
    return f"z[{var}] (an input)"


def _check(ctx, prog, input_sets, may_refuse=False):
    """run and run_many (1, 2, 3 batches, padded stride) == the model, bit for
    bit; returns False when create refused the program (only if may_refuse)"""
    from zelana_amd import gpu
    assert len(input_sets) == NB
    nv = prog.num_vars
    want = [M.limbs(M.interpret(prog, x)) for x in input_sets]
    stride = nv * 32 + 96
    # programs with kind 9 / 10 levels also run with one launch per level
    lean = bool(np.isin(prog.kinds, (POSEIDON_RC, SELECT)).any())
    for env in (None, "ZKMI_DEBUG_WPROG_NO_RC_CHAIN") if lean else (None,):
        wp = _open(ctx, prog, env)
        if wp is None:
            assert may_refuse, "zkmi_wprog_create refused a valid program"
            return False
        dz = gpu.DeviceBuffer(ctx, NB * stride)
        try:
            for nb in (0, 1, 2, 3):  # 0: zkmi_wprog_run
                dz.upload(np.full(NB * stride // 8, SENT, np.uint64))
                if nb == 0:
                    wp.run(input_sets[0], dz)
                else:
                    wp.run_many(input_sets[:nb], dz, stride)
                raw = dz.download(np.zeros((NB, stride // 8), np.uint64))
                how = f"run_many nb={nb}" if nb else "run"
                for i in range(max(nb, 1)):
                    got = raw[i, :nv * 4].reshape(nv, 4)
                    if not np.array_equal(got, want[i]):
                        bad = np.nonzero((got != want[i]).any(1))[0]
                        untouched = int((got[bad] == SENT).all(1).sum())
                        raise AssertionError(f"{how} batch {i}: {bad.size} of {nv} values differ ({untouched} never "
                                             f"written); first: {_what(prog, int(bad[0]))}, got "
                                             f"{M._ints(got[bad[0]])[0]:#x}, want {M._ints(want[i][bad[0]])[0]:#x}")
                    assert (raw[i, nv * 4:] == SENT).all(), f"{how} batch {i}: padding written"
                assert (raw[max(nb, 1):] == SENT).all(), f"{how}: wrote past its batches"
        finally:
            wp.close()
            dz.free()
    return True


# ------------------------------------------------------------ operand set E
def _rand(rng):
    return int.from_bytes(rng.bytes(32), "little") % R


def _top(k):
    """the largest value below r whose k low limbs (29 bits each) are all 0x1FFFFFFF"""
    return (((R >> (29 * k)) - 1) << (29 * k)) | ((1 << (29 * k)) - 1)


EDGE = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 2 ** 29 - 1, 2 ** 29, 2 ** 58, 2 ** 64 - 1, 2 ** 64,
        2 ** 232, 2 ** 253, _top(1), _top(2), _top(4), _top(8)]
NRAND = 3
LENGTHS = (3, 4, 5, 8, 9)


def _equal_to(v, length, y, rng, k):
    """a combination of `length` terms that equals z[v] only mod r, whatever
    z[v] and z[y] hold: terms on y that cancel (or carry coefficient 0), then
    terms on v whose coefficients (0, 1, r - 1 and random ones) sum to 1 + r"""
    b = _rand(rng)
    lc = [(y, 0)] if length % 2 else [(y, b), (y, R - b)]
    pool = [R - 1, _rand(rng), 1, 0, _rand(rng), R - 2, _rand(rng)]
    cs = [pool[(k + j) % len(pool)] for j in range(length - len(lc) - 1)]
    cs.append((1 - sum(cs)) % R)
    lc += [(v, c) for c in cs]
    assert len(lc) == length
    return lc[k % length:] + lc[:k % length]


class Operands:
    """Inputs One, 0, 1, then one slot per value of E; E itself as named
    combinations over them.  Batch b holds the values rotated by 5 b slots (and
    fresh random ones), so every slot sees an edge value in every batch."""

    def __init__(self, seed):
        self.rng = rng = np.random.default_rng(seed)
        n = len(EDGE) + NRAND
        self.slot = list(range(3, 3 + n))
        self.num_inputs = 3 + n
        self.values = [EDGE + [_rand(rng) for _ in range(NRAND)] for _ in range(NB)]
        x, y = self.slot[3], self.slot[-1]  # r - 1 and a random value in batch 0
        eight = [_rand(rng) for _ in range(7)]
        eight.append(-sum(eight) % R)
        self.zeros = [
            ("0: empty", []),
            ("0: 0 * c", [(ZERO, _rand(rng))]),
            ("0: x * 0", [(x, 0)]),
            ("0: x - x", [(x, 1), (x, R - 1)]),
            ("0: 1 + 0 - One", [(UNIT, 1), (ZERO, 1), (ONE, R - 1)]),
            ("0: 8 terms, coefficients summing to 0", [(y, c) for c in eight]),
        ]
        self.single = [(f"slot {i}", [(v, 1)]) for i, v in enumerate(self.slot)]
        self.multi = [(f"slot {i} in {LENGTHS[i % 5]} terms",
                       _equal_to(v, LENGTHS[i % 5], self.slot[(i + 7) % n], rng, i)) for i, v in enumerate(self.slot)]
        self.all = self.zeros + self.single + self.multi

    def inputs(self):
        n = len(self.slot)
        return [M.limbs([1, 0, 1] + [self.values[b][(i + 5 * b) % n] for i in range(n)]) for b in range(NB)]

    def reduced(self):
        """the zero forms and, as one input and as a combination, r - 1, r - 2,
        (r + 1) / 2, 2^64, 2^253, the all-ones limbs and a random value"""
        pick = [3, 4, 6, 11, 13, 17, len(EDGE)]
        return self.zeros + [self.single[i] for i in pick] + [self.multi[i] for i in pick]


def _program(E, ops, nvars, levels, **kw):
    """ops over E's inputs; levels = 2 puts the second half of the ops on a
    level of its own, so the two (small, permutation-free) levels are one
    k_wprog_chain launch and not a k_wprog_level launch each"""
    if levels == 2:
        ops = [o if i < len(ops) // 2 else o + (2,) for i, o in enumerate(ops)]
    prog = M.build(nvars, np.arange(E.num_inputs), ops, **kw)
    assert prog.num_levels == levels
    return prog


# (test_wprog_model_cpu.py checks, without a GPU, that E is what it claims to be)
# ------------------------------------------------------------ kinds over E
@pytest.mark.parametrize("levels", [1, 2])
def test_mul_pairs(ctx, levels):
    E = Operands(2)
    S = E.reduced()
    at, ops = E.num_inputs, []
    for _, a in S:
        for _, b in S:
            ops.append((MUL, at, 0, [a, b]))
            at += 1
    assert len(ops) == 400
    if levels == 2:  # two levels of 200: one chain launch
        assert len(ops) // 2 <= 256
    _check(ctx, _program(E, ops, at, levels), E.inputs())


@pytest.mark.parametrize("levels", [1, 2])
def test_inv_inv1_nz(ctx, levels):
    E = Operands(3)
    at, ops = E.num_inputs, []
    for j, (_, a) in enumerate(E.all):
        for kind in (INV, INV1, NZ)[j % 3:] + (INV, INV1, NZ)[:j % 3]:  # (the halves of levels = 2 hold all kinds)
            ops.append((kind, at, 0, [a]))
            at += 1
    assert len(ops) <= 256
    _check(ctx, _program(E, ops, at, levels), E.inputs())


@pytest.mark.parametrize("levels", [1, 2])
def test_bits64(ctx, levels):
    E = Operands(4)
    at, ops = E.num_inputs, []
    for _, a in E.all:
        ops.append((BITS64, at, 0, [a]))
        at += 64
    _check(ctx, _program(E, ops, at, levels), E.inputs())


WIDTHS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 253, 254, 256)


@pytest.mark.parametrize("levels", [1, 2])
def test_bits_widths(ctx, levels):
    E = Operands(5)
    operands = E.zeros + [E.single[3], E.multi[3], E.single[13], E.multi[13], E.single[-1], E.multi[-2]]
    at, ops = E.num_inputs, []
    for w in WIDTHS:
        for _, a in operands:
            ops.append((BITS, at, w, [a]))
            at += w
    assert len(ops) // 2 <= 256
    _check(ctx, _program(E, ops, at, levels), E.inputs())


def test_select(ctx):
    """conditions from E; t and f are combinations of several terms.  One
    level (k_wprog_level), two levels (k_wprog_chain's lean variant), and both
    again with the lean chain switched off (_check)"""
    for levels in (1, 2):
        E = Operands(6)
        rng, n = E.rng, len(E.slot)
        at, ops = E.num_inputs, []
        for j, (_, c) in enumerate(E.all):
            t = [(E.slot[j % n], _rand(rng)), (E.slot[(j + 3) % n], R - 1), (ONE, _rand(rng))]
            f = [(E.slot[(j + 1) % n], 1), (E.slot[(j + 2) % n], _rand(rng))] + ([(UNIT, R - 1)] if j % 2 else [])
            ops.append((SELECT, at, 0, [c, t if j % 7 else [], f if j % 5 else []]))
            at += 1
        _check(ctx, _program(E, ops, at, levels), E.inputs())


# --------------------------------------------------------------- PERM (MiMC)
def _root7(y):
    return pow(y, pow(7, -1, R - 1), R)  # x -> x^7 permutes Fr: 7 does not divide r - 1


def _perm_input_with_zero_round(k):
    """x whose round-k value t_k = t_{k-1}^7 + c_k is 0, solved backwards from round k"""
    t = 0
    for r in range(k, 0, -1):
        t = _root7((t - M.MIMC_C[r]) % R)
    return (t - M.MIMC_C[0]) % R


def test_perm_edges(ctx):
    rng = np.random.default_rng(7)
    vals = [0, R - 1, R - 2, _perm_input_with_zero_round(1), _perm_input_with_zero_round(3), _rand(rng), _rand(rng)]
    # the model agrees that these inputs hit t_r = 0: t_r^2 = 0 in the trace
    for x, r in ((R - 2, 0), (vals[3], 1), (vals[4], 3)):
        p1 = M.build(2 + 364, [0, 1], [(PERM, 2, 0, [[(1, 1)]])])
        assert M.interpret(p1, M.limbs([1, x]))[2 + 4 * r:2 + 4 * r + 4] == [0, 0, 0, 0]
    n = len(vals)
    nin = 3 + n
    at, ops, outs = nin, [], []
    for j in range(n):  # each slot as one input, three of them also as combinations
        forms = [[(3 + j, 1)]] + ([_equal_to(3 + j, LENGTHS[j % 5], 3 + (j + 1) % n, rng, j)] if j % 2 == 0 else [])
        for lc in forms:
            ops.append((PERM, at, 0, [lc]))
            outs.append(at + 4 * M.MIMC_ROUNDS - 1)
            at += 4 * M.MIMC_ROUNDS
    ops.append((PERM, at, 0, [[]]))  # the empty combination: MiMC of 0
    outs.append(at + 4 * M.MIMC_ROUNDS - 1)
    at += 4 * M.MIMC_ROUNDS
    for j, o in enumerate(outs):  # the outputs, read canonical by the next level
        ops.append((MUL, at, 0, [[(o, 1), (ONE, _rand(rng))], [(outs[(j + 1) % len(outs)], R - 1)]]))
        at += 1
    prog = M.build(at, np.arange(nin), ops)
    assert prog.level_sizes() == [len(outs), len(outs)]
    inputs = [M.limbs([1, 0, 1] + vals[2 * b:] + vals[:2 * b]) for b in range(NB)]
    _check(ctx, prog, inputs)


def test_create_refuses_reads_inside_a_mimc_trace(ctx):
    """all but the last of a PERM's 364 values are in Montgomery form while
    the program runs: an op that reads one is refused (ZKMI_EINVAL), not run
    on the wrong value; reading the output is accepted"""
    out = 3
    last = out + 4 * M.MIMC_ROUNDS - 1
    ops = [(PERM, out, 0, [[(1, 1)]]), (MUL, last + 1, 0, [[(last, 1)], [(2, 1)]])]
    prog = M.build(last + 2, [0, 1, 2], ops)
    row = int(np.nonzero(prog.term[:, 0] == last)[0][0])
    for var, accepted in ((last, True), (out, False), (out + 3, False), (last - 1, False), (last - 4, False)):
        prog.term[row, 0] = var
        wp = _open(ctx, prog)
        assert (wp is not None) == accepted, f"a read of trace value {var - out}"
        if wp is not None:
            wp.close()


# ------------------------------------------------ POSEIDON and POSEIDON_RC
def _poseidon_tables():
    from zelana_amd import shielded as S
    from zelana_amd.l2block import poseidon_params
    out = {}
    for kind, p in ((POSEIDON, poseidon_params()), (POSEIDON_RC, S.shielded_params())):
        out[kind] = (p["full"], p["partial"], [c for row in p["ark"] for c in row] + [c for row in p["mds"] for c in row])
    return out


def _poseidon_program(kind, table, rng):
    """Three permutations per mask 1..7; masked state elements cycle through
    0, r - 1, a random input, a lazy zero and a combination of several terms,
    unmasked ones through constant-only combinations (empty, One * c,
    One * (r - 1), One * 0); the next level reads every final x^5."""
    Z0, M1, A, B = 3, 4, 5, 6  # inputs after One, 0, 1: a 0, r - 1, two random values
    nin = 7
    var_forms = [[(Z0, 1)], [(M1, 1)], [(A, 1)], [(A, 1), (A, R - 1)],
                 [(A, _rand(rng)), (B, R - 1), (ONE, _rand(rng)), (M1, 1), (Z0, _rand(rng))]]
    const_forms = [[], [(ONE, _rand(rng))], [(ONE, R - 1)], [(ONE, 0)]]
    full, partial = table[0], table[1]
    at, ops, finals, k = nin, [], [], 0
    for mask in range(1, 8):
        for _ in range(3):
            lcs = []
            for q in range(3):
                k += 1
                lcs.append(var_forms[k % 5] if (mask >> q) & 1 else const_forms[k % 4])
            ops.append((kind, at, mask, lcs))
            n = M.poseidon_len(mask, full, partial)
            finals.append([at + n - 7, at + n - 4, at + n - 1])
            at += n
    for j, (x0, x1, x2) in enumerate(finals):
        if kind == POSEIDON_RC and j % 2:
            ops.append((SELECT, at, 0, [[(x0, 1)], [(x1, 1), (x2, R - 1)], [(x2, 1)]]))
        else:
            ops.append((MUL, at, 0, [[(x0, 1), (x1, _rand(rng))], [(x2, 1)]]))
        at += 1
    prog = M.build(at, np.arange(nin), ops, poseidon=table)
    assert prog.level_sizes() == [21, 21]
    inputs = [M.limbs([1, 0, 1, 0, R - 1, _rand(rng), _rand(rng)]) for _ in range(NB)]
    return prog, inputs


@pytest.mark.parametrize("kind", [POSEIDON, POSEIDON_RC])
def test_poseidon_masks_and_state_edges(ctx, kind):
    prog, inputs = _poseidon_program(kind, _poseidon_tables()[kind], np.random.default_rng(8 + kind))
    _check(ctx, prog, inputs)


# ------------------------------------------------------------ level geometry
class Levels:
    """Programs level by level: each level's ops read the values the previous
    level made (`prev`), so a level run early, late or not at all shows."""

    def __init__(self, seed, nfree=8):
        self.rng = np.random.default_rng(seed)
        self.nin = 3 + nfree
        self.at, self.lv, self.ops = self.nin, 0, []
        self.prev = list(range(3, self.nin))
        self.inputs = [M.limbs([1, 0, 1] + [_rand(self.rng) for _ in range(nfree)]) for _ in range(NB)]

    def _lc(self, i, n=2):
        p = self.prev
        return [(p[(i + 5 * k) % len(p)], (1, R - 1, _rand(self.rng))[(i + k) % 3]) for k in range(n)] + \
            [(ONE, _rand(self.rng))]

    def _emit(self, kind, extra, lcs, n_out=1):
        self.ops.append((kind, self.at, extra, lcs, self.lv))
        self.at += n_out
        return self.at - 1  # the op's last value

    def skip(self):  # an empty level
        self.lv += 1

    def cheap(self, n):
        """n MUL / NZ ops (every third an NZ, every ninth of a lazy zero)"""
        self.lv += 1
        outs = []
        for i in range(n):
            if i % 3 == 2:
                x = self.prev[i % len(self.prev)]
                outs.append(self._emit(NZ, 0, [[(x, 1), (x, R - 1)] if i % 9 == 8 else self._lc(i)]))
            else:
                outs.append(self._emit(MUL, 0, [self._lc(i), self._lc(i + 1, 1)]))
        self.prev = outs

    def select(self, n=1):
        """n SELECTs: a level the general chain does not take"""
        self.lv += 1
        self.prev = [self._emit(SELECT, 0, [self._lc(i, 1), self._lc(i + 1), self._lc(i + 2)]) for i in range(n)] + \
            self.prev[:4]

    def mixed(self):
        """INV, BITS, BITS64, NZ, INV1 and MUL in one level, twice over"""
        self.lv += 1
        outs = []
        for i in range(2):
            outs.append(self._emit(INV, 0, [self._lc(i)]))
            self._emit(BITS, 33, [self._lc(i + 1)], 33)
            self._emit(BITS64, 0, [[(self.prev[i], 1)]], 64)
            outs.append(self._emit(NZ, 0, [self._lc(i + 2)]))
            outs.append(self._emit(INV1, 0, [[(self.prev[i], 1), (self.prev[i], R - 1)]]))
            outs.append(self._emit(MUL, 0, [self._lc(i + 3), self._lc(i + 4)]))
        self.prev = outs

    def perms(self, n):
        self.lv += 1
        self.prev = [self._emit(PERM, 0, [self._lc(i)], 4 * M.MIMC_ROUNDS) for i in range(n)]

    def poseidons(self, kind, table, n):
        self.lv += 1
        outs = []
        for i in range(n):
            mask = (7, 5, 3, 6)[i % 4]
            lcs = [self._lc(i + q) if (mask >> q) & 1 else [(ONE, _rand(self.rng))] for q in range(3)]
            last = self._emit(kind, mask, lcs, M.poseidon_len(mask, table[0], table[1]))
            outs += [last - 6, last - 3, last]
        self.prev = outs

    def program(self, sizes, table=None):
        prog = M.build(self.at, np.arange(self.nin), self.ops, poseidon=table)
        assert prog.level_sizes() == sizes, prog.level_sizes()
        return prog


def test_level_sizes_in_one_run(ctx):
    """1, 63, 64, 65 and 256 ops: one chainable run; 257 ops: its own launch (two blocks and one quad)"""
    g = Levels(20)
    for n in (1, 63, 64, 65, 256, 257):
        g.cheap(n)
    _check(ctx, g.program([1, 63, 64, 65, 256, 257]), g.inputs)


def test_level_sizes_as_single_launches(ctx):
    """the same sizes, each between SELECT levels, so each is one k_wprog_level
    launch: 63 / 64 / 65 ops straddle its 64-op block, 256 / 257 the chain's limit"""
    g = Levels(21)
    sizes = []
    for n in (1, 63, 64, 65, 256, 257):
        g.cheap(n)
        g.select()
        sizes += [n, 1]
    _check(ctx, g.program(sizes), g.inputs)


def test_runs_of_one_two_three(ctx):
    """chainable runs of exactly 1, 2 and 3 levels between levels that are not (a SELECT level, a 257-op level)"""
    g = Levels(22)
    g.select()
    g.cheap(5)
    g.select(2)
    g.cheap(7)
    g.cheap(3)
    g.cheap(257)
    g.cheap(4)
    g.cheap(9)
    g.cheap(2)
    g.select()
    _check(ctx, g.program([1, 5, 2, 7, 3, 257, 4, 9, 2, 1]), g.inputs)


def test_big_level_splits_a_run(ctx):
    g = Levels(23)
    for n in (6, 11, 257, 5, 8):
        g.cheap(n)
    _check(ctx, g.program([6, 11, 257, 5, 8]), g.inputs)


def test_empty_level_inside_a_run(ctx):
    g = Levels(24)
    g.cheap(6)
    g.cheap(4)
    g.skip()
    g.cheap(5)
    g.cheap(3)
    g.skip()  # and an empty level before a single launch
    g.cheap(257)
    _check(ctx, g.program([6, 4, 0, 5, 3, 0, 257]), g.inputs)


def test_mixed_kinds_in_a_chain_and_alone(ctx):
    g = Levels(25)
    g.cheap(6)
    g.mixed()   # inside a chainable run
    g.cheap(5)
    g.select()
    g.mixed()   # its own launch
    g.select()
    _check(ctx, g.program([6, 12, 5, 1, 12, 1]), g.inputs)


def test_perm_level_then_chain(ctx):
    g = Levels(26)
    g.cheap(4)
    g.perms(3)
    g.cheap(6)  # reads the permutations' outputs
    g.cheap(5)
    g.cheap(2)
    _check(ctx, g.program([4, 3, 6, 5, 2]), g.inputs)


def test_kind7_level_then_chain(ctx):
    table = _poseidon_tables()[POSEIDON]
    g = Levels(27)
    g.cheap(4)
    g.poseidons(POSEIDON, table, 3)
    g.cheap(9)  # reads the final x^5 values
    g.cheap(5)
    _check(ctx, g.program([4, 3, 9, 5], table), g.inputs)


def test_lean_run_then_general_chain(ctx):
    """levels of kinds 9 and 10 alone (k_wprog_chain's lean variant) directly followed by a general chain"""
    table = _poseidon_tables()[POSEIDON_RC]
    g = Levels(28)
    g.poseidons(POSEIDON_RC, table, 2)
    g.select(3)
    g.poseidons(POSEIDON_RC, table, 1)
    g.cheap(7)
    g.cheap(4)
    g.select()
    _check(ctx, g.program([2, 3, 1, 7, 4, 1], table), g.inputs)


# ------------------------------------------------------ order inside a level
def _order_program(first, second, reader):
    """a level [first, second] in that order, then a level that reads the
    outputs of both: a MUL (the two levels are small: a chainable run when
    the first level is judged chainable) or a SELECT (every level its own
    launch)"""
    table = _poseidon_tables()[POSEIDON]
    g = Levels(30 + first + 3 * second + 7 * reader)
    g.lv = 1
    outs = []
    for kind in (first, second):
        if kind == MUL:
            outs.append(g._emit(MUL, 0, [g._lc(0), g._lc(1)]))
        elif kind == PERM:
            outs.append(g._emit(PERM, 0, [g._lc(2)], 4 * M.MIMC_ROUNDS))
        else:
            outs.append(g._emit(POSEIDON, 6, [[(ONE, 5)], g._lc(3), g._lc(4)], M.poseidon_len(6, 8, 56)))
    g.lv = 2
    lcs = [[(outs[0], 1), (outs[1], _rand(g.rng))], [(outs[1], 1)], [(outs[0], R - 1), (UNIT, 1)]]
    g._emit(reader, 0, lcs if reader == SELECT else lcs[:2])
    prog = M.build(g.at, np.arange(g.nin), g.ops, poseidon=table, keep_order=True)
    assert prog.level_sizes() == [2, 1] and prog.kinds.tolist() == [first, second, reader]
    return prog, g.inputs


@pytest.mark.parametrize("reader", [MUL, SELECT])
@pytest.mark.parametrize("first,second", [(MUL, PERM), (MUL, POSEIDON), (PERM, POSEIDON)])
def test_order_inside_a_level(ctx, first, second, reader):
    """zkmi.h: a level may hold its ops in any order.  The kernel of a level
    must come from all its ops, not from the first: a level [MUL, POSEIDON]
    launched without the Poseidon variant returns 0 and leaves the
    permutation's trace unwritten.  Either the model's z or ZKMI_EINVAL."""
    prog, inputs = _order_program(first, second, reader)
    _check(ctx, prog, inputs, may_refuse=True)
