"""R1CS satisfaction of resident witnesses on the GPU (zkmi_r1cs_check, the
prove path's check behind zkmi_ctx_set_prove_check / zkmi_groth16_last_check,
and the product layer above them).

Every expected status is a Python big-int evaluation of the rows done here
(_rows: cs.rows, or the CSR arrays of an R1CS made with set_csr), never the
library's.  Shapes are the smallest that cross the scan's edges: one row, either
side of a 256-row block, m + l = 2^10 exactly, both R1CS forms with long rows
(m = 33,000, the smallest that forces the legacy form), and a domain above
2^16 for the parts prove_many's wait submits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ host side
def _int(limbs) -> int:
    return sum(int(limbs[k]) << (64 * k) for k in range(4))


def _ints(arr):
    return [_int(v) for v in arr]


def _limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], np.uint64)


def _matrix(cs, name):
    """rows of (column, coefficient) as Python ints"""
    if cs.rows[name]:
        return cs.rows[name]
    rp, col, val = cs.csr(name)
    co, vi = [int(c) for c in col], _ints(val)
    return [[(co[k], vi[k]) for k in range(int(rp[i]), int(rp[i + 1]))] for i in range(cs.num_constraints)]


def _rows(mats, z):
    """(<a_i,z>, <b_i,z>, <c_i,z>) mod r for every row"""
    return [[sum(c * z[j] for j, c in row) % R for row in mat] for mat in mats]


def _status(a, b, c):
    from zelana_amd.gpu import R1CSStatus
    bad = [i for i in range(len(a)) if a[i] * b[i] % R != c[i]]
    if not bad:
        return R1CSStatus(None, 0, 0, 0, 0)
    f = bad[0]
    return R1CSStatus(f, len(bad), a[f], b[f], c[f])


def _expected(cs, z):
    return _status(*_rows([_matrix(cs, n) for n in "abc"], _ints(z) if isinstance(z, np.ndarray) else z))


def _break(z, cs, rows):
    """+1 on the product witness of each row (synthetic(satisfied=True): row i's
    lives in witness nv - m + i, which no A or B row reads)"""
    z = z.copy()
    nv, m = cs.num_variables, cs.num_constraints
    for i in rows:
        z[nv - m + i] = _limbs([(_int(z[nv - m + i]) + 1) % R])[0]
    return z


def _upload_many(ctx, zs, pad=0, fill=0):
    """the prove_many layout: assignment i at i * stride bytes, `pad` bytes of `fill` after each"""
    from zelana_amd import gpu
    nv = zs[0].shape[0]
    stride = nv * 32 + pad
    host = np.full((len(zs), stride // 8), fill, np.uint64)
    for i, z in enumerate(zs):
        host[i, :nv * 4] = z.reshape(-1)
    buf = gpu.DeviceBuffer(ctx, len(zs) * stride)
    buf.upload(host)
    return buf, stride


def _check_many(ctx, cs, zs, pad=0, fill=0):
    from zelana_amd import gpu
    dev = gpu.R1CSDevice(ctx, cs)
    buf, stride = _upload_many(ctx, zs, pad, fill)
    try:
        return gpu.r1cs_check(ctx, dev, buf, len(zs), stride)
    finally:
        buf.free()
        dev.close()


@pytest.fixture(scope="module")
def sat1021():
    """synthetic(1021, 3, 1100): m + l = 2^10 exactly; shared, never modified"""
    from zelana_amd.r1cs import synthetic
    return synthetic(1021, 3, 1100, seed=7, satisfied=True)


# ------------------------------------------------------------------ 1. stand-alone
@pytest.mark.parametrize("m,l,w", [(1, 1, 2), (255, 1, 300), (257, 3, 300), (1021, 3, 1100)])
def test_satisfied_and_single_breaks(ctx, m, l, w):
    from zelana_amd import gpu
    from zelana_amd.r1cs import synthetic
    cs, z = synthetic(m, l, w, seed=100 + m, satisfied=True)
    sets = []
    for s in ({0}, {m - 1}, {255, 256}, {7, 300, m - 1}):
        s = sorted(r for r in s if r < m)
        if s and s not in sets:
            sets.append(s)
    zs = [z] + [_break(z, cs, s) for s in sets]
    got = _check_many(ctx, cs, zs)
    assert got[0] == gpu.R1CSStatus(None, 0, 0, 0, 0) and got[0].ok
    for k, s in enumerate(sets):
        want = _expected(cs, zs[k + 1])
        assert (want.first_row, want.n_bad) == (s[0], len(s))  # (the break breaks those rows and nothing else)
        assert got[k + 1] == want, s
    # nb = 1, the default arguments
    dev, dz = gpu.R1CSDevice(ctx, cs), gpu.DeviceBuffer(ctx, z.nbytes)
    try:
        dz.upload(zs[-1])
        assert gpu.r1cs_check(ctx, dev, dz) == [_expected(cs, zs[-1])]
    finally:
        dz.free()
        dev.close()


def test_unsatisfied_everywhere(ctx):
    from zelana_amd.r1cs import synthetic_fast
    cs, z = synthetic_fast(1500, 4, 1600)
    want = _expected(cs, z)
    assert want.n_bad > 1400  # (random C: essentially every row)
    assert _check_many(ctx, cs, [z]) == [want]


def test_both_forms_and_long_rows(ctx):
    """A legacy (~100 K distinct coefficients), B and C compact (7 values
    including 1), 300 rows of 9-70 terms per matrix (lane groups) among short
    ones; C's last term of row i is a dedicated witness set so the row holds."""
    from zelana_amd.r1cs import R1CS, _rand_fr_array
    rng = np.random.default_rng(61)
    m, l, w = 33000, 5, 33100
    nv, free = l + w, l + w - m
    cs = R1CS(l, w)
    pool = _rand_fr_array(rng, 7)
    pool[0] = [1, 0, 0, 0]
    lens = {}
    for name in ("a", "b", "c"):
        ln = rng.integers(1, 5, size=m)
        ln[rng.choice(m, 300, replace=False)] = rng.integers(9, 71, size=300)
        rp = np.zeros(m + 1, np.uint64)
        rp[1:] = np.cumsum(ln)
        nnz = int(rp[-1])
        col = rng.integers(0, free, size=nnz, dtype=np.uint64)
        val = _rand_fr_array(rng, nnz) if name == "a" else pool[rng.integers(0, 7, size=nnz)]
        if name == "c":  # the row's last term: 1 x its dedicated witness
            col[rp[1:].astype(np.int64) - 1] = np.arange(nv - m, nv, dtype=np.uint64)
            val[rp[1:].astype(np.int64) - 1] = [1, 0, 0, 0]
        cs.set_csr(name, rp, col, val)
        lens[name] = ln
    cs._m = m
    zi = _ints(_rand_fr_array(rng, nv))
    zi[0] = 1
    for i in range(m):
        zi[nv - m + i] = 0
    mats = [_matrix(cs, n) for n in "abc"]
    a, b, c = _rows(mats, zi)
    for i in range(m):  # c_i = (rest of the row) + 1 x witness
        zi[nv - m + i] = (a[i] * b[i] - c[i]) % R
        c[i] = a[i] * b[i] % R
    short = next(i for i in range(m) if max(lens[n][i] for n in "abc") <= 8)
    long_ = next(i for i in range(m - 1, -1, -1) if lens["a"][i] > 8 and lens["c"][i] > 8)
    zs, want = [_limbs(zi)], [_status(a, b, c)]
    assert want[0].first_row is None
    for rows in ([short], [long_], [short, long_]):
        z2, c2 = list(zi), list(c)
        for i in rows:
            z2[nv - m + i] = (z2[nv - m + i] + 1) % R
            c2[i] = (c2[i] + 1) % R  # (the dedicated witness is read by C's row i alone)
        zs.append(_limbs(z2))
        want.append(_status(a, b, c2))
    assert [x.n_bad for x in want] == [0, 1, 1, 2]
    assert _check_many(ctx, cs, zs) == want


def test_range_edge(ctx):
    """Sums that are only congruent before the full reduction: 8 terms of 1 x
    (r - 1) sum lazily to 8 r - 8 = r - 8 mod r."""
    from zelana_amd import gpu
    from zelana_amd.r1cs import R1CS
    ONE, X, CW, ZW = 0, 1, 2, 3
    cs = R1CS(1, 3)
    cs.enforce([(X, 1)] * 8, [(ONE, 1)], [(CW, 1)])
    cs.enforce([], [(X, 1)], [])              # a = 0, c = 0
    cs.enforce([(ZW, 1)], [(X, 1)], [(ZW, 1)])  # the same through a zero witness
    cs.enforce([(X, 1)], [(ONE, 1)], [(X, 1)])  # a b = r - 1
    cs.enforce([(X, 1)], [(X, 1)], [(ONE, 1)])  # (r - 1)^2 = 1
    good, bad = [1, R - 1, R - 8, 0], [1, R - 1, R - 7, 0]
    got = _check_many(ctx, cs, [_limbs(good), _limbs(bad)])
    assert got[0] == gpu.R1CSStatus(None, 0, 0, 0, 0) == _expected(cs, good)
    assert got[1] == gpu.R1CSStatus(0, 1, R - 8, 1, R - 7) == _expected(cs, bad)


def test_batched_groups_and_arguments(ctx, sat1021):
    from zelana_amd import ZkmiError, gpu
    from zelana_amd.r1cs import _rand_fr_array
    cs, z = sat1021
    m, nv = cs.num_constraints, cs.num_variables
    rnd = _rand_fr_array(np.random.default_rng(3), nv)
    rnd[0] = [1, 0, 0, 0]
    zs = [z, _break(z, cs, [7]), z, _break(z, cs, [3, m - 1]), rnd]
    want = [_expected(cs, x) for x in zs]
    assert [(x.first_row, x.n_bad) for x in want[:4]] == [(None, 0), (7, 1), (None, 0), (3, 2)]
    assert want[4].n_bad > 1000
    for group in (2, 0):
        ctx.set_batch_group(group)
        try:
            assert _check_many(ctx, cs, zs, pad=96, fill=0xFFFFFFFFFFFFFFFF) == want, group
        finally:
            ctx.set_batch_group(0)
    dev = gpu.R1CSDevice(ctx, cs)
    buf, stride = _upload_many(ctx, zs[:2])
    try:
        assert gpu.r1cs_check(ctx, dev, buf, 0, stride) == []
        for bad_stride in (nv * 32 + 8, nv * 32 - 32):
            with pytest.raises(ZkmiError, match="z_stride"):
                gpu.r1cs_check(ctx, dev, buf, 1, bad_stride)
    finally:
        buf.free()
        dev.close()


# ------------------------------------------------------------------ 2. in the prove path
def _same(p, q):
    return all(np.array_equal(g, w) for g, w in zip(p, q))


def _random_zs(z0, count, seed):
    from zelana_amd.r1cs import _rand_fr_array
    rng = np.random.default_rng(seed)
    zs = [z0]
    for _ in range(count - 1):
        z = _rand_fr_array(rng, z0.shape[0])
        z[0] = [1, 0, 0, 0]
        zs.append(z)
    return zs


def test_prove_path_check(ctx, sat1021):
    """2^11 synthetic key over unsatisfied witnesses, 2^10 over satisfied and
    broken ones: proofs are the same bytes with the check on, and the statuses
    equal the stand-alone check's and the host evaluation."""
    from zelana_amd import gpu
    from zelana_amd.r1cs import synthetic_fast
    cs_u, z0 = synthetic_fast(1500, 4, 1600)
    cs_s, zsat = sat1021
    m = cs_s.num_constraints
    cases = [(cs_u, _random_zs(z0, 5, 9), gpu.synthetic_pk(ctx, 8, 11, 4, 1600)),
             (cs_s, [zsat, _break(zsat, cs_s, [7]), zsat, _break(zsat, cs_s, [3, m - 1]), _break(zsat, cs_s, [m - 1])],
              gpu.synthetic_pk(ctx, 9, 10, 3, 1100))]
    assert ctx.prove_check() is False
    for cs, zs, pk in cases:
        pk.precompute(0)
        dev = gpu.R1CSDevice(ctx, cs)
        buf, stride = _upload_many(ctx, zs, 64)
        rs, ss = [3, 5, 7, 9, 11], [4, 6, 8, 10, 12]
        want = [_expected(cs, z) for z in zs]
        try:
            ctx.set_batch_group(2)
            off1 = [gpu.groth16_prove_resident(ctx, pk, dev, buf.view(i * stride, stride), rs[i], ss[i])
                    for i in range(5)]
            assert gpu.groth16_last_check(ctx) == []
            offm = gpu.groth16_prove_many(ctx, pk, dev, buf, 5, stride, rs, ss)
            assert gpu.groth16_last_check(ctx) == []
            alone = gpu.r1cs_check(ctx, dev, buf, 5, stride)
            assert alone == want
            ctx.set_prove_check(True)
            assert ctx.prove_check() is True
            for i in range(5):
                on = gpu.groth16_prove_resident(ctx, pk, dev, buf.view(i * stride, stride), rs[i], ss[i])
                assert _same(on, off1[i]), i
                assert gpu.groth16_last_check(ctx) == [want[i]], i
            onm = gpu.groth16_prove_many(ctx, pk, dev, buf, 5, stride, rs, ss)
            assert all(_same(onm[i], offm[i]) and _same(onm[i], off1[i]) for i in range(5))
            assert gpu.groth16_last_check(ctx) == want
            # a single job, a batched one and a single one in flight together:
            # each reports its own statuses after its own wait
            j0 = gpu.groth16_prove_submit(ctx, pk, dev, buf.view(0, stride), rs[0], ss[0])
            jm = gpu.groth16_prove_many_submit(ctx, pk, dev, buf.view(stride, 3 * stride), 3, stride, rs[1:4], ss[1:4])
            ctx.set_prove_check(False)  # (j4 is submitted with the check off)
            j4 = gpu.groth16_prove_submit(ctx, pk, dev, buf.view(4 * stride, stride), rs[4], ss[4])
            assert _same(gpu.groth16_prove_wait(j0), off1[0])
            assert gpu.groth16_last_check(ctx) == want[:1]
            gm = gpu.groth16_prove_many_wait(jm)
            assert all(_same(gm[i], off1[1 + i]) for i in range(3))
            assert gpu.groth16_last_check(ctx) == want[1:4]
            assert _same(gpu.groth16_prove_wait(j4), off1[4])
            assert gpu.groth16_last_check(ctx) == []
        finally:
            ctx.set_prove_check(False)
            ctx.set_batch_group(0)
            buf.free()
            dev.close()
            pk.close()


def test_prove_many_above_small_schedule(ctx):
    """domain 2^17: the single-proof schedule with two in flight; the third
    proof is submitted by the wait and must use the flag the job sampled"""
    from zelana_amd import gpu
    from zelana_amd.r1cs import synthetic_fast
    cs, z0 = synthetic_fast(70000, 4, 70000)
    pk = gpu.synthetic_pk(ctx, 5, 17, 4, 70000)
    dev = gpu.R1CSDevice(ctx, cs)
    zs = _random_zs(z0, 3, 2)
    buf, stride = _upload_many(ctx, zs)
    mats = [_matrix(cs, n) for n in "abc"]
    want = [_status(*_rows(mats, _ints(z))) for z in zs]
    try:
        rs, ss = [11, 12, 13], [21, 22, 23]
        off = gpu.groth16_prove_many(ctx, pk, dev, buf, 3, stride, rs, ss)
        assert gpu.groth16_last_check(ctx) == []
        ctx.set_prove_check(True)
        job = gpu.groth16_prove_many_submit(ctx, pk, dev, buf, 3, stride, rs, ss)
        ctx.set_prove_check(False)
        on = gpu.groth16_prove_many_wait(job)
        got = gpu.groth16_last_check(ctx)
        assert len(got) == 3 and got == want
        assert all(_same(on[i], off[i]) for i in range(3))
        assert gpu.r1cs_check(ctx, dev, buf, 3, stride) == want
    finally:
        ctx.set_prove_check(False)
        buf.free()
        dev.close()
        pk.close()


# ------------------------------------------------------------------ 3. the product layer
def test_prover_check_flags_unsatisfied_batches():
    """Groth16Prover(check=True): honest L2 inputs are satisfied, the
    reference-style blake3 roots are not; the proofs are
    the same bytes as an unchecked prover's."""
    from test_gpu_l2block import _batch
    from zelana_amd.prover import Groth16Prover, l2_block_circuit
    p, _, _ = Groth16Prover.keygen(check=True)
    try:
        assert p.check is True
        honest, forged = _batch(41, 7, True), _batch(42, 100, False)
        cs, z = l2_block_circuit(*forged)
        want = _expected(cs, [int(v) for v in z])
        assert want.first_row is not None
        first = p.prove(*honest)  # (records the shape: host synthesis, then the resident proof)
        assert first.constraints_ok is True and first.first_unsatisfied is None
        ok, bad = p.prove(*honest), p.prove(*forged)
        assert ok.constraints_ok is True and ok.first_unsatisfied is None and ok.proof_bytes == first.proof_bytes
        assert bad.constraints_ok is False and bad.first_unsatisfied == want.first_row
        many = p.prove_many([honest, forged, forged, honest])
        assert [x.constraints_ok for x in many] == [True, False, False, True]
        assert [x.first_unsatisfied for x in many] == [None, want.first_row, want.first_row, None]
        r1 = p.prove_r1cs(cs, z, forged[0])
        assert r1.constraints_ok is False and r1.first_unsatisfied == want.first_row
        assert r1.proof_bytes == bad.proof_bytes
        p.check = False
        plain = p.prove(*forged)
        assert plain.constraints_ok is None and plain.first_unsatisfied is None
        assert plain.proof_bytes == bad.proof_bytes and p.prove(*honest).proof_bytes == ok.proof_bytes
        assert [x.constraints_ok for x in p.prove_many([honest, forged])] == [None, None]
    finally:
        p.pk.close()
        p.ctx.close()


def test_batch_worker_refuses_unsatisfied_batch(ctx):
    """ZBatchProver(check=True) raises for a batch whose public root does not
    match its witness, naming the row and the count; an honest batch gives the
    proof an unchecked worker gives."""
    from zelana_amd import batch_worker as BW
    from zelana_amd import gpu, zbatch as Z
    shape = dict(max_transfers=1, max_withdrawals=1, max_shielded=1, depth=2)
    d = Z.synthetic_batch(2, 1, seed=102)
    cs, z, _ = Z.build(d, **shape)
    n = 1
    while (1 << n) < cs.num_constraints + cs.num_instance:
        n += 1
    forged = dict(d)
    forged["post_state_root"] = (Z._f(d["post_state_root"]) + 1) % R
    _, zf, _ = Z.build(forged, **shape)
    want = _expected(cs, zf)
    assert want.first_row is not None and _expected(cs, z).first_row is None
    w = BW.ZBatchProver(ctx, d, pk=gpu.synthetic_pk(ctx, 3, n, cs.num_instance, cs.num_witness), check=True, **shape)
    try:
        res = w.generate_batch_proof(d)
        with pytest.raises(ValueError, match=rf"constraint {want.first_row} fails first, {want.n_bad} of "):
            w.generate_batch_proof(forged)
        assert ctx.prove_check() is False
        w.check = False
        assert w.generate_batch_proof(d).proof_bytes == res.proof_bytes
        assert len(w.generate_batch_proof(forged).proof_bytes) == 256
    finally:
        w.close()
        w.pk.close()
