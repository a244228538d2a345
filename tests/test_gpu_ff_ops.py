"""The device build of ff.h / ec.h (tests/device/ff_probe.hip over the op table
of tests/device/ff_ops.h: one lane per case, the op a uniform argument)
against the integer model of ff_model.py, with the case lists and the
assertions of test_ff_ops_cpu.py.

Every kernel outside wprog.hip computes with these routines, and only this
path runs the inline v_mad_u64_u32 of mac / macs / mac1 (FqP, FrP) and the
compiler-scheduled products that all G2 code uses (FqPn).  The cases of a
launch are shuffled, so the 64 lanes of a wave hold different operands and
different branches (generic sum, Q = P, Q = -P, infinity) side by side; no
launch is a multiple of 64 lanes and every one spans more than one block.

Field ops: exact limbs, normalised, inside the documented range.  Curve ops:
the model's affine point (or infinity, with *inf for xyzz_madd_g1f), the
"Out:" bounds, and limb for limb the host build's output, since both builds
run the same integer program.

Measured on an MI355X: 4.5 s for the whole file (97 tests, one launch per op
and field; nearly all of it is the Python model).  Cases per op, the lanes of
its launch (a/b where the fields' random values filter differently):
mul 11393, sqr 126, mul_add 784, sqr_add 4284, mul2 289, mul4 211, mul_x2
2646, sqr_x2 126, add 1025, sub 1025, dbl 65, neg 65, add_lazy 2305, subk2
5922/5930, subk4 6156/6172, subk6 6576/6593, subk8 6972/6988, reduce_q32 358,
reduce 65, is_zero 65, eq 1025, to_mont 65, from_mont 65, pack_unpack 65,
bsub_b2_1 65, bsub_b4_1 65, bsub_b8_1 65, bsub_b10_1 65, bsub2_b6_3 1025,
bsubadd_b10_1 1601, fq_cneg 65, f2_mul 972, f2_sqr 81, f2_mul_n 1452, f2_sqr_n
121, xyzz_madd_g1 451, xyzz_madd_g1f 897, xyzz_mmadd_g1 144, xyzz_add_g1 581,
xyzz_mdbl G1 65, xyzz_dbl G1 87, xyzz_madd G1 331, xyzz_add G1 581,
xyzz_madd_g2 451, xyzz_mmadd_g2 184, xyzz_add_g2 901, xyzz_mdbl G2 65,
xyzz_dbl G2 143, xyzz_madd G2 451, xyzz_add G2 901.
"""
import numpy as np
import pytest

import ff_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return M.load("libzkmi_ffprobe.so")


@pytest.fixture(scope="module")
def host():
    return M.load("libff_host.so")


FIELD_PARAMS = [(op, F) for F in M.FIELDS for op in M.field_ops_of(F)]
CURVE_PARAMS = [(op, G) for G in M.GROUPS for op in M.curve_ops_of(G)]


@pytest.mark.parametrize("op,F", FIELD_PARAMS, ids=[f"{op}-{F}" for op, F in FIELD_PARAMS])
def test_field_op(probe, op, F):
    cases = M.field_cases(op, F)
    assert cases.n > 64 and cases.n % 64
    out, flag = M.run(probe.ff_probe_field, F.id, M.FIELD_OPS.index(op), cases)
    M.check_field(op, F, cases, out, flag, "device")


@pytest.mark.parametrize("op,G", CURVE_PARAMS, ids=[f"{op}-{G}" for op, G in CURVE_PARAMS])
def test_curve_op(probe, host, op, G):
    cases = M.curve_cases(op, G)
    assert cases.n > 64 and cases.n % 64
    out, flag = M.run(probe.ff_probe_curve, G.id, M.CURVE_OPS.index(op), cases, G.width)
    M.check_curve(op, G, cases, out, flag, "device")
    hout, hflag = M.run(host.ff_host_curve, G.id, M.CURVE_OPS.index(op), cases, G.width)
    bad = np.nonzero((out != hout).any(axis=(1, 2)) | (flag != hflag))[0]
    assert bad.size == 0, (f"{op} {G}: device and host limbs differ in {bad.size} lanes, first lane {bad[0]} "
                           f"({cases.what[bad[0]]}): device {out[bad[0]].tolist()} flag {flag[bad[0]]}, "
                           f"host {hout[bad[0]].tolist()} flag {hflag[bad[0]]}")


def test_unsupported_ops_are_refused(probe):
    """an op a field does not have is refused before any HIP call"""
    assert probe.ff_probe_field(2, M.FIELD_OPS.index("mul_x2"), None, None, None, 0) == -1
    assert probe.ff_probe_field(1, M.FIELD_OPS.index("fq_cneg"), None, None, None, 0) == -1
    assert probe.ff_probe_curve(1, M.CURVE_OPS.index("xyzz_madd_g1f"), None, None, None, 0) == -1
