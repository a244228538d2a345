"""ff.h's mad blocks (ZK_MAD_BLOCKS, the default: a column's v_mad_u64_u32 as
one asm statement) against its one-mad statements, and the G1 table MSM's
items path built on them against the CPU oracle.

The op table of tests/device/ff_ops.h is built twice (build_native.py):
libzkmi_ffprobe.so with the blocks and libzkmi_ffprobe_1mad.so with
-DZK_MAD_BLOCKS=0.  Every routine of the table runs the full case lists of
ff_model.py (the contract-edge representatives among them) through both, and
the output words and flags must be equal: a block sums the terms of its
column in another order, which may not show in any limb.  (test_gpu_ff_ops.py
checks the default build against the integer model.)

The MSM is the smallest plan that takes the one-lane-per-bucket accumulation
(table window 19: 2^18 buckets) over 2^13 bases, on one lane and on two: it
runs k_acc_items_g1, k_split_combine, the strip reduction and the bit sums.
"""
import numpy as np
import pytest

import ff_model as M
import oracle_ctypes as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blocks():
    return M.load("libzkmi_ffprobe.so")


@pytest.fixture(scope="module")
def one_mad():
    return M.load("libzkmi_ffprobe_1mad.so")


FIELD_PARAMS = [(op, F) for F in M.FIELDS for op in M.field_ops_of(F)]
CURVE_PARAMS = [(op, G) for G in M.GROUPS for op in M.curve_ops_of(G)]


def _same(what, cases, a, b):
    (out_a, flag_a), (out_b, flag_b) = a, b
    bad = np.nonzero((out_a != out_b).any(axis=(1, 2)) | (flag_a != flag_b))[0]
    assert bad.size == 0, (f"{what}: the two builds differ in {bad.size} lanes, first lane {bad[0]} "
                           f"({cases.what[bad[0]]}): blocks {out_a[bad[0]].tolist()} flag {flag_a[bad[0]]}, "
                           f"one-mad {out_b[bad[0]].tolist()} flag {flag_b[bad[0]]}")


@pytest.mark.parametrize("op,F", FIELD_PARAMS, ids=[f"{op}-{F}" for op, F in FIELD_PARAMS])
def test_field_op_same_words(blocks, one_mad, op, F):
    cases = M.field_cases(op, F)
    assert cases.n > 64 and cases.n % 64
    op_id = M.FIELD_OPS.index(op)
    _same(f"{op}<{F}>", cases, M.run(blocks.ff_probe_field, F.id, op_id, cases),
          M.run(one_mad.ff_probe_field, F.id, op_id, cases))


@pytest.mark.parametrize("op,G", CURVE_PARAMS, ids=[f"{op}-{G}" for op, G in CURVE_PARAMS])
def test_curve_op_same_words(blocks, one_mad, op, G):
    cases = M.curve_cases(op, G)
    assert cases.n > 64 and cases.n % 64
    op_id = M.CURVE_OPS.index(op)
    _same(f"{op} {G}", cases, M.run(blocks.ff_probe_curve, G.id, op_id, cases, G.width),
          M.run(one_mad.ff_probe_curve, G.id, op_id, cases, G.width))


# ------------------------------------------------------------ the items path
N = 1 << 13
WINDOW = 19  # 2^18 buckets: the smallest plan with one lane per bucket (ITEMS_MIN_K)


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(ctx):
    """2^13 bases with one at infinity, one repeated (P + P in a bucket) and
    one beside its negation (P + (-P)), as a window-19 table; two scalar
    vectors over a pool of 32 values, and the oracle's sum for each."""
    pts = O.gen_points_g1(1913, N)
    pts[3] = 0                          # infinity
    pts[101] = pts[100]                 # P, P
    pts[201] = pts[200]                 # P, -P
    y = O.limbs_to_int(pts[200, 4:])
    pts[201, 4:] = O.int_to_limbs(O.Q - y)
    pool = O.gen_scalars(1914, 32)
    rng = np.random.default_rng(1915)
    vectors = []
    for _ in range(2):
        # values 0 and 1 of the pool go to one base and to two, the other 30
        # to ~270 each: a window's buckets hold 0, 1, 2 and many entries
        pick = rng.integers(2, 32, N)
        pick[[7, 100, 101]] = (0, 1, 1)
        pick[[200, 201]] = 5            # the pair that cancels shares its buckets with many others
        pick[[300, 301]] = 6
        vectors.append(np.ascontiguousarray(pool[pick]))
    pts[301] = pts[300]                 # P + P inside a long bucket as well
    b = ctx.bases_g1(pts)
    info = b.precompute(WINDOW, 0)
    assert info[1] == WINDOW
    return b, vectors, [O.msm_g1(pts, sc) for sc in vectors]


def test_items_path_one_lane(ctx, table):
    b, vectors, want = table
    keep = ctx.lanes()
    ctx.set_lanes(1)
    try:
        for sc, w in zip(vectors, want):
            assert np.array_equal(ctx.msm(b, sc), w)
    finally:
        ctx.set_lanes(keep)


def test_items_path_two_lanes(ctx, table):
    """two MSMs in flight, one a lane: an accumulation beside the other
    lane's sort and reduction"""
    from zelana_amd.gpu import DeviceBuffer
    b, vectors, want = table
    dev = []
    for sc in vectors:
        d = DeviceBuffer(ctx, sc.nbytes)
        d.upload(sc)
        dev.append(d)
    keep = ctx.lanes()
    ctx.set_lanes(2)
    try:
        jobs, got = [], []
        for i in range(4):
            jobs.append(ctx.msm_submit(b, dev[i & 1], N))
            if len(jobs) == 2:
                got.append(ctx.msm_wait(jobs.pop(0)))
        got += [ctx.msm_wait(j) for j in jobs]
    finally:
        ctx.set_lanes(keep)
    for i, g in enumerate(got):
        assert np.array_equal(g, want[i & 1]), f"MSM {i} of 4 in flight on two lanes"
