"""Batched proving on the GPU (zkmi_msm_batch_*, zkmi_ntt_batch_device,
zkmi_groth16_prove_many, Groth16Prover.prove_many): every batched result must
equal, limb for limb, the single-item entry point on the same input, and the
oracle where the size allows.  Shapes are the smallest that cross each path
boundary of msm.hip / ntt.hip (SMALL_SORT_MAX = 2^18 entries, CUTSUM_COOP_K =
2^16 buckets, single-workgroup NTT below 2^11, two / three NTT groups)."""
import ctypes

import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_groth16 import _oracle_prove, _setup

pytestmark = pytest.mark.gpu

R = O.R
NPTS = 3000


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. NTT
@pytest.mark.parametrize("log_n", [3, 10, 11, 13, 17])
def test_ntt_batch(ctx, log_n):
    from zelana_amd import gpu
    n = 1 << log_n
    base = O.gen_scalars(100 + log_n, 3 * n).reshape(3, n, 4)
    for nb in (1, 3):
        for pad in (0, 64):
            stride = n * 32 + pad
            host = np.full((nb, stride // 8), 0xA5A5A5A5A5A5A5A5, np.uint64)
            for i in range(nb):
                host[i, :n * 4] = base[i].reshape(-1)
            buf = gpu.DeviceBuffer(ctx, nb * stride)
            one = gpu.DeviceBuffer(ctx, n * 32)
            try:
                for inverse in (False, True):
                    for coset in (False, True):
                        buf.upload(host)
                        ctx.ntt_batch_device(buf, log_n, nb, stride, inverse, coset)
                        got = buf.download(np.zeros_like(host))
                        for i in range(nb):
                            one.upload(base[i])
                            ctx.ntt_device(one, log_n, inverse, coset)
                            want = one.download(np.zeros((n, 4), np.uint64))
                            assert np.array_equal(got[i, :n * 4].reshape(n, 4), want), (nb, pad, inverse, coset, i)
                            if log_n <= 13:
                                assert np.array_equal(want, O.ntt(base[i], log_n, inverse, coset))
                            assert np.all(got[i, n * 4:] == np.uint64(0xA5A5A5A5A5A5A5A5)), "pad bytes written"
            finally:
                buf.free()
                one.free()


# ------------------------------------------------------------------ 2. MSM
def _kinds(n, seed):
    """the scalar vectors of the issue: uniform, all zero, all ones, all r - 1, 0/1 witness-like"""
    rng = np.random.default_rng(seed)
    one = np.zeros((n, 4), np.uint64)
    one[:, 0] = 1
    rm1 = np.tile(np.array(O.int_to_limbs(R - 1), np.uint64), (n, 1))
    bits = np.zeros((n, 4), np.uint64)
    bits[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint64)
    return [O.gen_scalars(seed, n).reshape(n, 4), np.zeros((n, 4), np.uint64), one, rm1, bits]


def _vectors(n, nb, seed):
    ks = _kinds(n, seed)
    vs = [ks[i % 5] if i < 5 else O.gen_scalars(seed + i, n).reshape(n, 4) for i in range(nb)]
    if nb >= 7:
        vs[6] = vs[0]  # two identical vectors
    return vs


@pytest.fixture(scope="module")
def sets(ctx):
    """per group: oracle points and the plain / full-table / partial-table base sets over them"""
    out = {}
    for g2 in (False, True):
        pts = (O.gen_points_g2 if g2 else O.gen_points_g1)(2020 if g2 else 1020, NPTS)
        mk = ctx.bases_g2 if g2 else ctx.bases_g1
        plain, full, part = mk(pts), mk(pts), mk(pts)
        assert full.precompute(13, 0)[1:] == (13, 20, 1)
        part.precompute(13, 3)
        big = ctx.bases_generate(7, 20000, g2)
        out[g2] = dict(pts=pts, plain=plain, full=full, part=part, big=big)
    return out


def _run_batch(ctx, bases, vs, n, pad, offset=0, pts=None):
    """msm_batch over the vectors == msm_device_n on each (== the oracle when pts is given)"""
    from zelana_amd import gpu
    nb, stride = len(vs), n * 32 + pad
    host = np.zeros((max(nb, 1), stride // 8), np.uint64)
    for i, v in enumerate(vs):
        host[i, :n * 4] = v.reshape(-1)
    buf = gpu.DeviceBuffer(ctx, max(nb, 1) * stride)
    buf.upload(host)
    try:
        got = ctx.msm_batch(bases, buf, n, nb, stride, offset)
        assert got.shape == (nb, 16 if bases.g2 else 8)
        for i in range(nb):
            want = ctx.msm_device_n(bases, buf.view(i * stride, n * 32), n, offset)
            assert np.array_equal(got[i], want), f"vector {i} of {nb}"
            if pts is not None:
                ref = (O.msm_g2 if bases.g2 else O.msm_g1)(pts[offset:offset + n], vs[i])
                assert np.array_equal(want, ref)
        return got
    finally:
        buf.free()


# (name, base set, n, nb, window, group, pad, offset)
MSM_CASES = [
    ("radix_c8", "plain", 700, 3, 8, 64, 0, 0),
    ("plain_auto_c13", "big", 20000, 2, 0, 64, 64, 0),
    # 11 bin-sort chunks per vector (the last partial) x 3 vectors = 33 > 32 super-chunks, so they pair up
    # and super-chunk 5 holds the last chunk of vector 0 and the first of vector 1
    ("bin_sort_superchunk_across_vectors", "big", 11000, 3, 13, 64, 64, 0),
    ("table_counting_sort", "full", 3000, 4, 0, 64, 0, 0),
    ("table_bin_sort", "full", 3000, 5, 0, 64, 64, 0),
    ("table_small_split_K16", "full", 700, 16, 0, 64, 0, 0),
    ("table_cascade_K17", "full", 700, 17, 0, 64, 0, 0),
    ("partial_table", "part", 3000, 4, 0, 64, 0, 0),
    ("offset", "full", 1000, 3, 0, 64, 64, 1234),
    ("group_2_of_5", "full", 700, 5, 0, 2, 0, 0),
    ("group_auto", "full", 700, 5, 0, 0, 0, 0),
]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("case", MSM_CASES, ids=[c[0] for c in MSM_CASES])
def test_msm_batch(ctx, sets, case, g2):
    name, which, n, nb, window, group, pad, offset = case
    s = sets[g2]
    ctx.set_window(window)
    ctx.set_batch_group(group)
    try:
        vs = _vectors(n, nb, 31 + nb)
        got = _run_batch(ctx, s[which], vs, n, pad, offset, s["pts"] if which != "big" else None)
        assert not got[1].any(), "all-zero scalars give infinity"
        if nb >= 7:
            assert np.array_equal(got[6], got[0])
    finally:
        ctx.set_window(0)
        ctx.set_batch_group(0)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_msm_batch_edges(ctx, sets, g2):
    from zelana_amd import gpu
    from zelana_amd._lib import lib
    s = sets[g2]
    w = 16 if g2 else 8
    n, nb = 700, 3
    vs = _vectors(n, nb, 5)
    buf = gpu.DeviceBuffer(ctx, nb * n * 32)
    buf.upload(np.stack(vs))
    try:
        assert ctx.msm_batch(s["full"], buf, n, 0, n * 32).shape == (0, w)           # nb = 0
        assert not ctx.msm_batch(s["full"], buf, 0, nb, n * 32).any()                # n = 0: infinity
        want = [ctx.msm_device_n(s["full"], buf.view(i * n * 32, n * 32), n) for i in range(nb)]
        out = np.zeros((nb + 1, w), np.uint64)
        p64 = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        # zkmi_msm_wait on a batch job and a wrong nb: ZKMI_EINVAL, the job still finishes after
        job = ctx.msm_batch_submit(s["full"], buf, n, nb, n * 32)
        assert lib().zkmi_msm_wait(job[0], p64) == -1
        assert lib().zkmi_msm_batch_wait(job[0], p64, nb + 1) == -1
        assert np.array_equal(ctx.msm_batch_wait(job), np.stack(want))
        # zkmi_msm_batch_wait on a single job
        single = ctx.msm_submit(s["full"], buf, n)
        assert lib().zkmi_msm_batch_wait(single[0], p64, 1) == -1
        assert np.array_equal(ctx.msm_wait(single), want[0])
    finally:
        buf.free()


# ------------------------------------------------------------------ 3. prove
def _upload_many(ctx, zs, pad=0):
    from zelana_amd import gpu
    nv = zs[0].shape[0]
    stride = nv * 32 + pad
    host = np.zeros((len(zs), stride // 8), np.uint64)
    for i, z in enumerate(zs):
        host[i, :nv * 4] = z.reshape(-1)
    buf = gpu.DeviceBuffer(ctx, len(zs) * stride)
    buf.upload(host)
    return buf, stride


def _check_prove_many(ctx, cs, zs, seed):
    """plain key and precompute(0), group automatic and 2: every proof == the oracle's == prove_resident's"""
    from zelana_amd import gpu
    opk, pkb, rng, (st, keep) = _setup(cs, seed)
    nb = len(zs)
    rs, ss = [rng.fr() for _ in range(nb)], [rng.fr() for _ in range(nb)]
    want = [_oracle_prove(opk, st, zs[i], rs[i], ss[i]) for i in range(nb)]
    pk = gpu.ProvingKey(ctx, pkb, True)
    dev = gpu.R1CSDevice(ctx, cs)
    buf, stride = _upload_many(ctx, zs, 64)
    try:
        for table in (False, True):
            if table:
                pk.precompute(0)
            for i in range(nb):
                got = gpu.groth16_prove_resident(ctx, pk, dev, buf.view(i * stride, stride), rs[i], ss[i])
                assert all(np.array_equal(g, w) for g, w in zip(got, want[i])), ("resident", table, i)
            for group in (0, 2):
                ctx.set_batch_group(group)
                many = gpu.groth16_prove_many(ctx, pk, dev, buf, nb, stride, rs, ss)
                ctx.set_batch_group(0)
                for i in range(nb):
                    assert all(np.array_equal(g, w) for g, w in zip(many[i], want[i])), (table, group, i)
    finally:
        ctx.set_batch_group(0)
        buf.free()
        dev.close()
        pk.close()
        O.lib().oracle_pk_free(opk)


def test_prove_many_matches_oracle_2e11(ctx):
    from zelana_amd.r1cs import _rand_fr_array, synthetic_fast
    cs, z0 = synthetic_fast(1500, 4, 1600)
    rng = np.random.default_rng(9)
    zs = [z0]
    for _ in range(4):
        z = _rand_fr_array(rng, z0.shape[0])
        z[0] = [1, 0, 0, 0]
        zs.append(z)
    _check_prove_many(ctx, cs, zs, 1500)


def test_prove_many_satisfied_small_domain(ctx):
    """2^7 domain: the single-workgroup NTT, tables with c < 12, the compacted B queries"""
    from zelana_amd.r1cs import synthetic
    m, l, w = 100, 3, 120
    cs, z0 = synthetic(m, l, w, seed=103, satisfied=True)
    nv = l + w
    rng = np.random.default_rng(4)
    zs = [z0]
    for _ in range(2):
        z = [1] + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(nv - 1)]
        for i in range(m):  # the product witnesses of the new free values
            av = sum(c * z[j] for j, c in cs.rows["a"][i]) % R
            bv = sum(c * z[j] for j, c in cs.rows["b"][i]) % R
            z[nv - m + i] = av * bv % R
        assert cs.is_satisfied(z)
        zs.append(np.array([O.int_to_limbs(v) for v in z], np.uint64))
    _check_prove_many(ctx, cs, zs, m)


# ------------------------------------------------------------------ 4. above the small schedule
def test_prove_many_large_domain(ctx):
    from zelana_amd import gpu
    from zelana_amd.r1cs import _rand_fr_array, synthetic_fast
    cs, z0 = synthetic_fast(70000, 4, 70000)  # m + l > 2^16: domain 2^17
    pk = gpu.synthetic_pk(ctx, 5, 17, 4, 70000)
    dev = gpu.R1CSDevice(ctx, cs)
    rng = np.random.default_rng(2)
    zs = [z0]
    for _ in range(2):
        z = _rand_fr_array(rng, z0.shape[0])
        z[0] = [1, 0, 0, 0]
        zs.append(z)
    buf, stride = _upload_many(ctx, zs)
    try:
        rs, ss = [11, 12, 13], [21, 22, 23]
        many = gpu.groth16_prove_many(ctx, pk, dev, buf, 3, stride, rs, ss)
        for i in range(3):
            one = gpu.groth16_prove_resident(ctx, pk, dev, buf.view(i * stride, stride), rs[i], ss[i])
            assert all(np.array_equal(g, w) for g, w in zip(many[i], one)), i
    finally:
        buf.free()
        dev.close()
        pk.close()


# ------------------------------------------------------------------ 5. the product path
def test_prover_prove_many_equals_prove():
    from test_gpu_l2block import _batch
    from zelana_amd.prover import Groth16Prover
    p, _, _ = Groth16Prover.keygen()
    try:
        spec = [(0, 100, True), (41, 7, True), (42, 100, False), (0, 100, True)]
        batches = [_batch(*s) for s in spec]
        many = p.prove_many(batches)
        assert [m.public_inputs.batch_id for m in many] == [s[0] for s in spec]
        for m, (inp, w) in zip(many, batches):
            one = p.prove(inp, w)
            assert m.proof_bytes == one.proof_bytes and len(m.proof_bytes) == 256
            assert np.array_equal(m.a, one.a) and np.array_equal(m.b, one.b) and np.array_equal(m.c, one.c)
    finally:
        p.pk.close()
        p.ctx.close()


# ------------------------------------------------------------------ 6. interleaving
def test_single_and_batched_jobs_interleave(ctx):
    """single submit, prove_many submit, single submit, then the waits in order:
    lanes, workspaces and sort counter blocks are reused across plan sizes"""
    from zelana_amd import gpu
    from zelana_amd.r1cs import _rand_fr_array, synthetic_fast
    cs, z0 = synthetic_fast(1500, 4, 1600)
    pk = gpu.synthetic_pk(ctx, 8, 11, 4, 1600)
    pk.precompute(0)
    dev = gpu.R1CSDevice(ctx, cs)
    rng = np.random.default_rng(6)
    zs = [z0]
    for _ in range(4):
        z = _rand_fr_array(rng, z0.shape[0])
        z[0] = [1, 0, 0, 0]
        zs.append(z)
    buf, stride = _upload_many(ctx, zs)
    try:
        rs, ss = [3, 5, 7, 9, 11], [4, 6, 8, 10, 12]
        alone = [gpu.groth16_prove_resident(ctx, pk, dev, buf.view(i * stride, stride), rs[i], ss[i])
                 for i in range(5)]
        j0 = gpu.groth16_prove_submit(ctx, pk, dev, buf.view(0, stride), rs[0], ss[0])
        jm = gpu.groth16_prove_many_submit(ctx, pk, dev, buf.view(stride, 3 * stride), 3, stride, rs[1:4], ss[1:4])
        j4 = gpu.groth16_prove_submit(ctx, pk, dev, buf.view(4 * stride, stride), rs[4], ss[4])
        got = [gpu.groth16_prove_wait(j0)] + gpu.groth16_prove_many_wait(jm) + [gpu.groth16_prove_wait(j4)]
        for i in range(5):
            assert all(np.array_equal(g, w) for g, w in zip(got[i], alone[i])), i
    finally:
        buf.free()
        dev.close()
        pk.close()
