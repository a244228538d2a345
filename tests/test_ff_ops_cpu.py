"""The host build of ff.h / ec.h (tests/native/ff_host_shim.cpp over the op
table of tests/device/ff_ops.h) against the integer model of ff_model.py, one
op and field at a time, at the edges of each op's written contract.

This leg validates the model and the case lists without a GPU;
test_gpu_ff_ops.py runs the same lists through the device build.

Field ops: the output limbs equal the model's limbs exactly, limbs 0..7 are
normalised and the value lies inside the op's documented range.  Curve ops:
to_affine(output) is the model's point or both are infinity, and every output
coordinate meets the op's "Out:" line.

xyzz_madd_g1f's `z == 0 || e == 0` test (PP == 0 or PP == p exactly): with
P = U2 - X1 + 8p = REDC(x2 ZZ1) + (8p - X1) and X1 < 8p, P is never 0, so
Q = +-P means P = k p with 1 <= k <= 9, and REDC(k^2 p^2) =
(k^2 p^2 + (R - k^2 p) p) / R = p exactly (k^2 p < R up to k = 13).  Every
Q = +-P case below therefore takes the `e == 0` arm (with every k that
X1 = x + k p, k = 0..7, produces), and the `z == 0` arm is unreachable inside
the contract: it would need X1 = 8p.
"""
import pytest

import ff_model as M


@pytest.fixture(scope="module")
def host():
    return M.load("libff_host.so")


FIELD_PARAMS = [(op, F) for F in M.FIELDS for op in M.field_ops_of(F)]
CURVE_PARAMS = [(op, G) for G in M.GROUPS for op in M.curve_ops_of(G)]


def test_op_table_is_covered():
    """every op of ff_ops.h runs for at least one field / group, and has a contract"""
    assert {op for op, _ in FIELD_PARAMS} == set(M.FIELD_OPS)
    assert {op for op, _ in CURVE_PARAMS} == set(M.CURVE_OPS)
    for op in M.FIELD_OPS + M.CURVE_OPS:
        assert op in M.CONTRACT or op[:4] in M.CONTRACT, op


def test_unsupported_ops_are_refused(host):
    for F in M.FIELDS:
        for i, op in enumerate(M.FIELD_OPS):
            if op not in M.field_ops_of(F):
                assert host.ff_host_field(F.id, i, None, None, None, 0) == -1
    assert host.ff_host_field(0, len(M.FIELD_OPS), None, None, None, 0) == -1
    assert host.ff_host_curve(1, M.CURVE_OPS.index("xyzz_madd_g1"), None, None, None, 0) == -1
    assert host.ff_host_curve(0, len(M.CURVE_OPS), None, None, None, 0) == -1


def test_spread_and_borrow_forms():
    for F in (M.FQ, M.FR):
        for v in M.wide_values(F, 32):
            for lim in (M.L30, M.L15, M.L31):
                assert M.val(M.spread(v, lim)) == v
        x = M.spread((6 << 232) - 1, M.L31)
        assert min(x[:8]) >= M.L31 - 4  # the saturated value reaches the limit in every limb
    # FqP's borrow-form constants: limb-wise non-negative against what they are subtracted from
    assert min(M.borrow_form(M.FQ, 8, 1)[:8]) >= M.L29
    assert min(M.borrow_form(M.FQ, 6, 3)[:8]) >= 3 * M.L29


@pytest.mark.parametrize("op,F", FIELD_PARAMS, ids=[f"{op}-{F}" for op, F in FIELD_PARAMS])
def test_field_op(host, op, F):
    cases = M.field_cases(op, F)
    assert cases.n > 64 and cases.n % 64
    out, flag = M.run(host.ff_host_field, F.id, M.FIELD_OPS.index(op), cases)
    M.check_field(op, F, cases, out, flag, "host")


@pytest.mark.parametrize("op,G", CURVE_PARAMS, ids=[f"{op}-{G}" for op, G in CURVE_PARAMS])
def test_curve_op(host, op, G):
    cases = M.curve_cases(op, G)
    assert cases.n > 64 and cases.n % 64
    out, flag = M.run(host.ff_host_curve, G.id, M.CURVE_OPS.index(op), cases, G.width)
    M.check_curve(op, G, cases, out, flag, "host")


def test_madd_g1f_cancellation_takes_the_pp_equals_p_arm():
    """the argument of the module docstring on the model: for Q = +-P the fast
    mixed addition's PP is exactly p, for every representative of X1"""
    F = M.FQ
    cases = M.curve_cases("xyzz_madd_g1f", M.G1)
    hits = 0
    for i in range(cases.n):
        x = [tuple(int(l) for l in r) for r in cases.inp[i]]
        b8x = tuple((c - a) & 0xFFFFFFFF for c, a in zip(M.borrow_form(F, 8, 1), x[0]))
        pp_ = M.field_model("mul_add", F, [x[4], x[2], b8x], 0)[0][0]
        pp = M.val(M.field_model("sqr", F, [pp_], 0)[0][0])
        same_x = M.val(pp_) % M.Q == 0
        assert (pp == M.Q) == same_x and pp != 0
        hits += same_x
        want = cases.want[i]
        if same_x:  # Q = P or Q = -P
            P = M.G1.to_affine(*M.curve_out(M.G1, cases.inp[i, :4]))
            assert want is None or want == M.G1.add(P, P)
    assert hits > 100


def test_mul_with_both_factors_at_1p5_2_30_leaves_the_contract(host):
    """ff.h's header once read "mul accepts inputs < 8p with limbs < 1.5 2^30".
    With both factors there a column holds 8 products of up to 2.25 2^60 and
    wraps 2^64, so the host build leaves the model: the contract is the finer
    one (both < 2^30 for a single product), which test_field_op[mul-*] holds at
    its limit.  Host only: the case is outside the contract the GPU lists keep."""
    for F in (M.FQ, M.FR):
        a = M.spread((6 << 232) - 1, M.L15)
        rows = [[a, a]] * 65
        cases = M.Cases(rows, [0] * 65, ["saturated"] * 65)
        out, _ = M.run(host.ff_host_field, F.id, M.FIELD_OPS.index("mul"), cases)
        want = M.field_model("mul", F, [a, a], 0)[0][0]
        assert tuple(int(l) for l in out[0, 0]) != want
        # the same value at the contract's limit is exact
        b = M.spread((6 << 232) - 1, M.L30)
        cases = M.Cases([[b, b]] * 65, [0] * 65, ["saturated"] * 65)
        out, _ = M.run(host.ff_host_field, F.id, M.FIELD_OPS.index("mul"), cases)
        assert tuple(int(l) for l in out[0, 0]) == M.field_model("mul", F, [b, b], 0)[0][0]


def test_subk_first_operand_at_2_31_leaves_the_contract(host):
    """subk's comment once allowed limbs "up to 2^31" for both operands.  The
    pass forms a_i + (K p)_i unsigned and reads it as int32, so a limb of a
    near 2^31 turns negative and the carry comes out 8 short: a's limbs go up
    to 1.5 2^30 (what ntt.hip passes; test_field_op[subk*] holds that limit
    and b's 2^31), not further.  Host only, as the case is outside the
    contract."""
    for F in (M.FQ, M.FR):
        a, b = M.spread((6 << 232) - 1, M.L31), M.norm(1)
        cases = M.Cases([[a, b]] * 65, [0] * 65, ["saturated"] * 65)
        out, _ = M.run(host.ff_host_field, F.id, M.FIELD_OPS.index("subk2"), cases)
        assert tuple(int(l) for l in out[0, 0]) != M.field_model("subk2", F, [a, b], 0)[0][0]
