"""Plain-integer model of zelana_amd/csrc/ff.h and ec.h, and the case lists
that tests/test_ff_ops_cpu.py (host build) and tests/test_gpu_ff_ops.py
(device build) run through the op table of tests/device/ff_ops.h.

An element is 9 limbs of 29 bits, v(x) = sum x_i 2^(29 i), Montgomery radix
R = 2^261.  Every ff.h routine is a deterministic function on integers, so
the model predicts the exact output limbs from the mathematics (REDC, a
difference plus K p, a quotient estimate), never by walking limbs as ff.h does;
only the routines ff.h itself defines limb-wise (add_lazy, bsub*) are limb-wise
here.  CONTRACT holds each op's input contract as ff.h / ec.h write it next to
the op; the case builders stay inside it and go to its edges.
"""
import numpy as np

NL, LB = 9, 29
MASK = (1 << LB) - 1
RAD = 1 << (NL * LB)  # Montgomery radix 2^261
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M_Q32 = (1 << 48) // (0x30644E + 2)  # reduce_q32's quotient multiplier (top limb of q and r, + 2)
L29, L30, L15, L31 = 1 << 29, 1 << 30, 3 << 29, 1 << 31  # limb limits the contracts name
SEED = 0x5EED_FF


class Field:
    def __init__(self, name, fid, p):
        self.name, self.id, self.p = name, fid, p
        self.pinv = (-pow(p, -1, RAD)) % RAD
        self.one = RAD % p
        self.r2 = RAD * RAD % p

    def __repr__(self):
        return self.name


FQ, FR, FQN = Field("FqP", 0, Q), Field("FrP", 1, R), Field("FqPn", 2, Q)
FIELDS = (FQ, FR, FQN)


# ------------------------------------------------------------------ limbs
def val(x):
    return sum(int(l) << (LB * i) for i, l in enumerate(x))


def norm(v):
    """normalised limbs of v >= 0: limbs 0..7 < 2^29, limb 8 the rest mod 2^32"""
    assert v >= 0
    return tuple((v >> (LB * i)) & MASK for i in range(NL - 1)) + ((v >> (LB * (NL - 1))) & 0xFFFFFFFF,)


def spread(v, limit):
    """The representation of v whose limbs 0..7 are raised as far as `limit`
    (exclusive, a multiple of 2^29) and v allow: from the top down, each limb
    borrows up to limit / 2^29 - 1 units of the limb above it."""
    x = list(norm(v))
    m = limit // L29 - 1
    for i in range(NL - 2, -1, -1):
        t = min(m, x[i + 1])
        x[i] += t << LB
        x[i + 1] -= t
    assert val(x) == v and all(l < limit for l in x[:NL - 1])
    return tuple(x)


def borrow_form(F, k, m):
    """BK_m of ff.h: K p with limbs 0..7 raised by m 2^29, m borrowed from the limb above"""
    x = list(norm(k * F.p))
    for i in range(NL - 1):
        x[i] += m << LB
        x[i + 1] -= m
    assert val(x) == k * F.p
    return tuple(x)


# ------------------------------------------------------------- field model
def redc(F, t):
    return (t + ((t * F.pinv) % RAD) * F.p) >> (NL * LB)


def _plus_d(s, d):
    """a Montgomery result s with the addend d folded into its upper columns"""
    s += val(d[:NL - 1])
    return norm(s)[:NL - 1] + (((s >> (LB * (NL - 1))) + d[NL - 1]) & 0xFFFFFFFF,)


def m_mul(F, a, b):
    return norm(redc(F, val(a) * val(b)))


def m_add(F, a, b):
    s = val(a) + val(b)
    return norm(s - 2 * F.p if s >= 2 * F.p else s)


def m_sub(F, a, b):
    s = val(a) - val(b)
    return norm(s + 2 * F.p if s < 0 else s)


def m_add_lazy(a, b):
    return tuple((x + y) & 0xFFFFFFFF for x, y in zip(a, b))


def m_subk(F, k, a, b):
    return norm(val(a) - val(b) + k * F.p)


def m_reduce(F, a):
    v = val(a)
    return norm(v - F.p if v >= F.p else v)


def m_reduce_q32(F, x):
    return norm(val(x) - ((x[NL - 1] * M_Q32) >> 48) * F.p)


def field_model(op, F, x, flag):
    """(output limb tuples, flag or None) of op on the input limb tuples x"""
    p = F.p
    v = [val(t) for t in x]
    if op == "mul":
        return (m_mul(F, x[0], x[1]),), None
    if op == "sqr":
        return (norm(redc(F, v[0] * v[0])),), None
    if op == "mul_add":
        return (_plus_d(redc(F, v[0] * v[1]), x[2]),), None
    if op == "sqr_add":
        return (_plus_d(redc(F, v[0] * v[0]), x[1]),), None
    if op == "mul2":
        return (norm(redc(F, v[0] * v[1] + v[2] * v[3])),), None
    if op == "mul4":
        return (norm(redc(F, v[0] * v[1] + v[2] * v[3] + v[4] * v[5] + v[6] * v[7])),), None
    if op == "mul_x2":
        return (m_mul(F, x[0], x[1]), m_mul(F, x[2], x[3])), None
    if op == "sqr_x2":
        return (m_mul(F, x[0], x[0]), m_mul(F, x[1], x[1])), None
    if op == "add":
        return (m_add(F, x[0], x[1]),), None
    if op == "sub":
        return (m_sub(F, x[0], x[1]),), None
    if op == "dbl":
        return (m_add(F, x[0], x[0]),), None
    if op == "neg":
        return (m_sub(F, norm(0), x[0]),), None
    if op == "add_lazy":
        return (m_add_lazy(x[0], x[1]),), None
    if op.startswith("subk"):
        return (m_subk(F, int(op[4:]), x[0], x[1]),), None
    if op == "reduce_q32":
        return (m_reduce_q32(F, x[0]),), None
    if op == "reduce":
        return (m_reduce(F, x[0]),), None
    if op == "is_zero":
        return (), int(v[0] % p == 0)
    if op == "eq":
        return (), int((v[0] - v[1]) % p == 0)
    if op == "to_mont":
        return (m_mul(F, x[0], norm(F.r2)),), None
    if op == "from_mont":
        return (m_reduce(F, m_mul(F, x[0], norm(1))),), None
    if op == "pack_unpack":
        return (norm(v[0] % (1 << 256)),), None
    if op.startswith("bsub_"):
        c = borrow_form(F, *_BK[op])
        return (tuple((ci - ai) & 0xFFFFFFFF for ci, ai in zip(c, x[0])),), None
    if op == "bsub2_b6_3":
        c = borrow_form(F, 6, 3)
        return (tuple((ci - (ai + 2 * bi)) & 0xFFFFFFFF for ci, ai, bi in zip(c, x[0], x[1])),), None
    if op == "bsubadd_b10_1":
        c = borrow_form(F, 10, 1)
        return (tuple((ci - ai + bi) & 0xFFFFFFFF for ci, ai, bi in zip(c, x[0], x[1])),), None
    if op == "fq_cneg":
        return (norm(2 * p - v[0]) if flag else tuple(x[0]),), None
    if op == "f2_mul":
        t0, t1 = m_mul(F, x[0], x[2]), m_mul(F, x[1], x[3])
        t2 = m_mul(F, m_add_lazy(x[0], x[1]), m_add_lazy(x[2], x[3]))
        return (m_sub(F, t0, t1), m_sub(F, m_sub(F, t2, t0), t1)), None
    if op == "f2_sqr":
        c1 = m_mul(F, x[0], x[1])
        return (m_mul(F, m_add_lazy(x[0], x[1]), m_sub(F, x[0], x[1])), m_add(F, c1, c1)), None
    if op == "f2_mul_n":
        return (norm(redc(F, v[0] * v[2] + v[1] * (4 * p - v[3]))), norm(redc(F, v[0] * v[3] + v[1] * v[2]))), None
    if op == "f2_sqr_n":
        return (norm(redc(F, (v[0] + v[1]) * (v[0] - v[1] + 4 * p))), norm(redc(F, 2 * v[0] * v[1]))), None
    raise KeyError(op)


_BK = {"bsub_b2_1": (2, 1), "bsub_b4_1": (4, 1), "bsub_b8_1": (8, 1), "bsub_b10_1": (10, 1)}

# op -> ids in the order of ff_ops.h's FieldOp / CurveOp
FIELD_OPS = ["mul", "sqr", "mul_add", "sqr_add", "mul2", "mul4", "mul_x2", "sqr_x2", "add", "sub", "dbl", "neg",
             "add_lazy", "subk2", "subk4", "subk6", "subk8", "reduce_q32", "reduce", "is_zero", "eq", "to_mont",
             "from_mont", "pack_unpack", "bsub_b2_1", "bsub_b4_1", "bsub_b8_1", "bsub_b10_1", "bsub2_b6_3",
             "bsubadd_b10_1", "fq_cneg", "f2_mul", "f2_sqr", "f2_mul_n", "f2_sqr_n"]
CURVE_OPS = ["xyzz_madd_g1", "xyzz_madd_g1f", "xyzz_mmadd_g1", "xyzz_add_g1", "xyzz_madd_g2", "xyzz_mmadd_g2",
             "xyzz_add_g2", "xyzz_mdbl", "xyzz_dbl", "xyzz_madd", "xyzz_add"]
N_OUT = {"mul_x2": 2, "sqr_x2": 2, "is_zero": 0, "eq": 0, "f2_mul": 2, "f2_sqr": 2, "f2_mul_n": 2, "f2_sqr_n": 2}


def field_ops_of(F):
    """the ops of ff_ops.h's field_op_supported for F"""
    out = []
    for op in FIELD_OPS:
        if op in ("mul_x2", "sqr_x2"):
            ok = F is not FQN
        elif op.startswith("bsub") or op == "fq_cneg":
            ok = F is FQ
        elif op.startswith("f2_"):
            ok = F is FQN
        else:
            ok = True
        if ok:
            out.append(op)
    return out


# The input contracts, as ff.h / ec.h state them beside each routine.
CONTRACT = {
    "mul": "a b < 169 p^2 (R / p = 169.3); limbs of both factors < 2^30 (a single product), or of one "
           "< 1.5 2^30 and the other normalised",
    "sqr": "a^2 < 169 p^2; limbs < 2^30",
    "mul_add": "a, b as mul; d: limbs 0..7 < 2^31, limb 8 added modulo 2^32; value < a b / R + p + d",
    "sqr_add": "as mul_add with b = a",
    "mul2": "a, c: limbs < 2^30; b, d: limbs < 2^29; or (xyzz_madd_g1f) a normalised, b limbs < 1.5 2^30, "
            "c limbs < 2^30, d normalised; a b + c d < 169 p^2",
    "mul4": "all limbs < 2^29; a b + c d + e f + g h < 169 p^2",
    "mul_x2": "two independent mul",
    "sqr_x2": "two independent sqr",
    "add": "a, b in [0, 2p), normalised -> [0, 2p)",
    "sub": "a, b in [0, 2p), normalised -> [0, 2p)",
    "dbl": "add(a, a)",
    "neg": "sub(0, a)",
    "add_lazy": "limb-wise, no carry: limbs of the sum < 2^32 (callers: < 2^31, value < 6p)",
    "subk": "0 <= a - b + K p < 2^261; limbs of a < 1.5 2^30, limbs of b < 2^31",
    "reduce_q32": "x in [0, 32p), limbs 0..7 < 2^31 -> [0, 2p)",
    "reduce": "[0, 2p) normalised -> [0, p)",
    "is_zero": "[0, 2p) normalised",
    "eq": "[0, 2p) normalised",
    "to_mont": "canonical value (any normalised value < 2p is inside mul's contract)",
    "from_mont": "[0, 2p) normalised -> canonical [0, p)",
    "pack_unpack": "normalised, value < 2^256",
    "bsub": "a normalised; the difference K p - a may borrow in limb 8 only",
    "bsub2_b6_3": "a, b normalised (a + 2b per limb < 3 2^29)",
    "bsubadd_b10_1": "a, b normalised; limbs of the result < 1.5 2^30",
    "fq_cneg": "y < 2p normalised -> 2p - y (in (0, 2p]) or y",
    "f2_mul": "components in [0, 2p), normalised",
    "f2_sqr": "components in [0, 2p), normalised",
    "f2_mul_n": "components normalised, values < 4p -> < 2p",
    "f2_sqr_n": "components normalised, values < 4p -> < 2p",
    "xyzz_madd_g1": "p.x < 8p, p.y/zz/zzz < 2p, q < 2p (p may be infinity) -> x < 8p, y/zz/zzz < 2p",
    "xyzz_madd_g1f": "p finite, p.x < 8p, p.y/zz/zzz < 2p normalised; qx < 2p normalised; qy value < 2p, "
                     "limbs < 2^30 -> x < 8p, y/zz/zzz < 2p; *inf when Q == -P",
    "xyzz_mmadd_g1": "p, q affine < 2p -> as xyzz_madd_g1",
    "xyzz_add_g1": "all coordinates < 2p normalised (either may be infinity) -> < 2p",
    "xyzz_madd_g2": "all coordinates < 2p normalised (p may be infinity) -> < 2p",
    "xyzz_mmadd_g2": "p, q affine < 2p -> < 2p",
    "xyzz_add_g2": "all coordinates < 2p normalised (either may be infinity) -> < 2p",
    "xyzz_mdbl": "affine < 2p -> < 2p",
    "xyzz_dbl": "coordinates < 2p (may be infinity) -> < 2p",
    "xyzz_madd": "coordinates < 2p (p may be infinity) -> < 2p",
    "xyzz_add": "coordinates < 2p (either may be infinity) -> < 2p",
}


def out_bound(op, F, x, flag):
    """exclusive upper bound of every output value that the op documents"""
    p = F.p
    if op in ("reduce", "from_mont"):
        return p
    if op in ("mul_add", "sqr_add"):
        b = x[0] if op == "sqr_add" else x[1]
        d = x[2] if op == "mul_add" else x[1]
        d8 = d[NL - 1] - (1 << 32) if d[NL - 1] >> 31 else d[NL - 1]  # a borrow in limb 8 of a difference
        return val(x[0]) * val(b) // RAD + p + val(d[:NL - 1]) + (d8 << (LB * (NL - 1))) + 1
    if op.startswith("subk"):
        return RAD
    if op == "fq_cneg":
        return 2 * p + 1
    if op == "add_lazy" or op.startswith("bsub"):
        return None  # limb-wise forms: the limbs are the contract
    if op == "pack_unpack":
        return 1 << 256
    return 2 * p


# ------------------------------------------------------------- field cases
class Cases:
    """n cases: inp (n, 8, W) u32, flag (n,) u32, what[i] a description of case i"""

    def __init__(self, rows, flags, what, width=NL, seed=0):
        n = len(rows)
        assert n > 0
        # more than one 64-lane block, and no multiple of 64: repeat leading cases
        extra = 0
        while (n + extra) <= 64 or (n + extra) % 64 == 0:
            extra += 1
        idx = list(range(n)) + [i % n for i in range(extra)]
        rng = np.random.default_rng(SEED + seed)
        idx = [idx[i] for i in rng.permutation(len(idx))]  # a wave's 64 lanes hold different operands
        self.rows = [rows[i] for i in idx]
        self.what = [what[i] for i in idx]
        self.n = len(idx)
        self.inp = np.zeros((self.n, 8, width), np.uint32)
        for i, r in enumerate(self.rows):
            for s, t in enumerate(r):
                self.inp[i, s] = t
        self.flag = np.array([flags[i] for i in idx], np.uint32)


def _rand_below(rng, bound):
    return int.from_bytes(rng.bytes(40), "little") % bound


def base_values(F):
    """the value set of every op: all < 2p"""
    p = F.p
    rng = np.random.default_rng(SEED + F.id)
    vs = [0, 1, 2, p - 1, p, p + 1, 2 * p - 1, (p - 1) // 2, F.one, F.r2, 1 << 253, 1 << 254, (1 << 29) - 1,
          (1 << 232) - 1, 1 << 232, (6 << 232) - 1]  # the last: limbs 0..7 all ones and a top limb to borrow from
    return vs + [_rand_below(rng, 2 * p) for _ in range(16)]


def wide_values(F, kmax, ks=None):
    """base values and k p + e for every k below kmax (or the k of ks, for the
    operand lists whose cross product is taken): all < kmax p"""
    p = F.p
    return base_values(F) + [k * p + e for k in (ks or range(2, kmax)) for e in (0, 1, p - 1)]


def reps(values, limits):
    """(limbs, description) of each value normalised and spread to each limit"""
    out = []
    for v in values:
        seen = set()
        for lim in (L29,) + tuple(limits):
            x = norm(v) if lim == L29 else spread(v, lim)
            if x not in seen:
                seen.add(x)
                out.append((x, f"{v:#x}@{lim / L30:g}*2^30"))
    return out


def _edge_values(F):
    p = F.p
    return [0, 1, p - 1, p, 2 * p - 1, F.one, (6 << 232) - 1] + base_values(F)[16:20]


def field_cases(op, F):
    p = F.p
    ZERO = norm(0)
    rows, flags, what = [], [], []

    def put(ops, flag=0):
        rows.append([o[0] for o in ops])
        flags.append(flag)
        what.append(", ".join(o[1] for o in ops))

    if op == "mul":
        A = reps(wide_values(F, 13, (2, 3, 7, 8, 9, 12)), (L30,))
        for a in A:
            for b in A:
                if val(a[0]) * val(b[0]) < 169 * p * p:
                    put((a, b))
        for a in reps(wide_values(F, 10, (8, 9)), (L15,)):  # one factor a limb-wise sum of three
            for b in reps(base_values(F), ()):
                if a[0] != norm(val(a[0])):
                    put((a, b))
                    put((b, a))
    elif op == "sqr":
        for a in reps(wide_values(F, 13), (L30,)):
            put((a,))
    elif op in ("mul_add", "sqr_add"):
        # d: normalised, limb-wise sums up to 2^31, and the borrow forms K p - x
        D = reps(wide_values(F, 10), (L30, L31))
        D += [(tuple((c - a) & 0xFFFFFFFF for c, a in zip(borrow_form(F, k, 1), norm(v))), f"B{k}_1-{v:#x}")
              for k in (4, 8) for v in base_values(F)[:16] + [k * p - 1]]
        if op == "sqr_add":
            for a in reps(wide_values(F, 13, (2, 7, 9, 12)), (L30,)):
                for d in D[::5] + D[2::17]:
                    put((a, d))
        else:
            A = reps(_edge_values(F) + [k * p + e for k in (7, 8) for e in (0, p - 1)], (L30,))
            i = 0
            for a in A:
                for b in A:
                    if val(a[0]) * val(b[0]) < 169 * p * p:
                        put((a, b, D[i % len(D)]))  # every pair, the addends in turn
                        i += 1
    elif op == "mul2":
        S = _edge_values(F) + [k * p + e for k in (3, 8, 9) for e in (0, p - 1)]
        pairs = [(a, b) for a in S for b in S]
        rng = np.random.default_rng(SEED + 2)
        other = rng.permutation(len(pairs))
        for i, (a, b) in enumerate(pairs):
            c, d = pairs[other[i]]
            if a * b + c * d >= 169 * p * p:
                continue
            if i % 2:  # xyzz_madd_g1f: R normalised, Q - X3 + 10p < 1.5 2^30; 4p - Y1 < 2^30, PPP normalised
                put((reps([a], ())[0], reps([b], (L15,))[-1], reps([c], (L30,))[-1], reps([d], ())[0]))
            else:      # a, c < 2^30; b, d < 2^29
                put((reps([a], (L30,))[-1], reps([b], ())[0], reps([c], (L30,))[-1], reps([d], ())[0]))
    elif op == "mul4":
        B = base_values(F)
        rng = np.random.default_rng(SEED + 4)
        for _ in range(200):
            put(reps([B[j] for j in rng.integers(0, len(B), 8)], ()))
        h = 13 * p // 2  # four products of 6.5p x 6.5p: 169 p^2
        for d in (1, 2, p // 3, p - 1):
            put(reps([h - d] * 8, ()))
            put(reps([h, h, h, h, h, h, h, h - d], ()))
        lim = 169 * p * p
        for a, b in ((13 * p - 1, 13 * p - 1), (12 * p + 1, 14 * p), (2 * p - 1, 84 * p)):
            rest = lim - a * b - 1  # the other products bring the sum to one below the bound
            c = 2 * p - 1
            put(reps([a, b, c, rest // c, 1, rest % c, 0, 0], ()))
    elif op in ("mul_x2", "sqr_x2"):
        A = reps(wide_values(F, 13), (L30,))
        rng = np.random.default_rng(SEED + 6)
        if op == "sqr_x2":
            o = rng.permutation(len(A))
            for i, a in enumerate(A):
                put((a, A[o[i]]))
        else:
            P2 = [(a, b) for a in A[::2] for b in A[1::3] if val(a[0]) * val(b[0]) < 169 * p * p]
            o = rng.permutation(len(P2))
            for i, (a, b) in enumerate(P2):
                put((a, b) + P2[o[i]])
    elif op in ("add", "sub", "eq"):
        A = reps(base_values(F), ())
        for a in A:
            for b in A:
                put((a, b))
    elif op in ("dbl", "neg", "reduce", "is_zero", "to_mont", "from_mont"):
        for a in reps(base_values(F), ()):
            put((a,))
    elif op == "add_lazy":
        for a in reps(wide_values(F, 4), (L30,)):
            for b in reps(base_values(F), ()):
                put((a, b))
    elif op.startswith("subk"):
        k = int(op[4:])
        A = reps(wide_values(F, 10, (2, 3, 7, 9)) + [RAD - k * p - 1, RAD - 1], (L15,))
        B = reps(wide_values(F, 10, (2, 5, 7, 9)) + [RAD - 1], (L31,))
        for a in A:
            for b in B:
                if 0 <= val(a[0]) - val(b[0]) + k * p < RAD:
                    put((a, b))
    elif op == "reduce_q32":
        for a in reps(wide_values(F, 32), (L30, L31)):
            put((a,))
    elif op == "pack_unpack":
        for a in reps(base_values(F) + [(1 << 255), (1 << 256) - 1, (1 << 256) - (1 << 232)], ()):
            put((a,))
    elif op.startswith("bsub_"):
        k = _BK[op][0]
        for a in reps([v for v in wide_values(F, k + 1) if v <= k * p], ()):
            put((a,))
    elif op == "bsub2_b6_3":  # 6p - PPP - 2Q: normalised products < 2p
        A = reps(base_values(F), ())
        for a in A:
            for b in A:
                put((a, b))
    elif op == "bsubadd_b10_1":  # 10p - X3 + Q: X3 < 8p, Q < 2p
        for a in reps(wide_values(F, 8), ()):
            for b in reps(base_values(F), ()):
                put((a, b))
    elif op == "fq_cneg":
        for a in reps(base_values(F), ()):
            put((a,), 0)
            put((a,), 1)
    elif op.startswith("f2_"):
        V = (_edge_values(F)[:6] + base_values(F)[16:19]) if op in ("f2_mul", "f2_sqr") else \
            (_edge_values(F)[:6] + base_values(F)[16:18] + [2 * p, 3 * p + 1, 4 * p - 1])
        E = [(a, b) for a in reps(V, ()) for b in reps(V, ())]
        if op.endswith("sqr") or op.endswith("sqr_n"):
            for a in E:
                put(a)
        else:
            rng = np.random.default_rng(SEED + 8)
            for a in E:
                for j in rng.integers(0, len(E), 12):
                    put(a + E[j])
    else:
        raise KeyError(op)
    return Cases(rows, flags, what, NL, seed=FIELD_OPS.index(op))


# ------------------------------------------------------------------ curves
class Fp1:
    """arithmetic of Fq on ints"""
    zero, one, b = 0, 1, 3
    add = staticmethod(lambda a, b: (a + b) % Q)
    sub = staticmethod(lambda a, b: (a - b) % Q)
    mul = staticmethod(lambda a, b: a * b % Q)
    inv = staticmethod(lambda a: pow(a, -1, Q))
    scale = staticmethod(lambda a, k: a * k % Q)


class Fp2:
    """arithmetic of Fq2 = Fq[u] / (u^2 + 1) on pairs of ints"""
    zero, one = (0, 0), (1, 0)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q))
    mul = staticmethod(lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q))
    scale = staticmethod(lambda a, k: (a[0] * k % Q, a[1] * k % Q))

    @staticmethod
    def inv(a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
        return (a[0] * n % Q, -a[1] * n % Q)


Fp2.b = Fp2.mul((3, 0), Fp2.inv((9, 1)))  # the twist y^2 = x^3 + 3 / (9 + u)


class Group:
    def __init__(self, name, gid, K, gen):
        self.name, self.id, self.K, self.gen = name, gid, K, gen
        self.width = NL if K is Fp1 else 2 * NL
        assert self.on_curve(gen)

    def __repr__(self):
        return self.name

    def on_curve(self, P):
        K = self.K
        return K.mul(P[1], P[1]) == K.add(K.mul(K.mul(P[0], P[0]), P[0]), K.b)

    def neg(self, P):
        return None if P is None else (P[0], self.K.sub(self.K.zero, P[1]))

    def add(self, P, S):
        """affine group law; None is the point at infinity"""
        K = self.K
        if P is None:
            return S
        if S is None:
            return P
        if P[0] == S[0]:
            if P[1] != S[1] or P[1] == K.zero:
                return None
            lam = K.mul(K.scale(K.mul(P[0], P[0]), 3), K.inv(K.scale(P[1], 2)))
        else:
            lam = K.mul(K.sub(S[1], P[1]), K.inv(K.sub(S[0], P[0])))
        x = K.sub(K.sub(K.mul(lam, lam), P[0]), S[0])
        return (x, K.sub(K.mul(lam, K.sub(P[0], x)), P[1]))

    def mul(self, k, P=None):
        acc, P = None, self.gen if P is None else P
        while k:
            if k & 1:
                acc = self.add(acc, P)
            P = self.add(P, P)
            k >>= 1
        return acc

    # coordinates <-> limb rows: a G1 coordinate is one element, a G2 one is c0 then c1
    def comps(self, c):
        return (c,) if self.K is Fp1 else tuple(c)

    def coord(self, cs):
        return cs[0] if self.K is Fp1 else tuple(cs)

    def to_affine(self, X, Y, ZZ, ZZZ):
        """the affine point of Montgomery-form XYZZ values (x = X / ZZ, y = Y / ZZZ:
        the Montgomery factors cancel); None when ZZ = 0 mod p"""
        K = self.K
        red = lambda c: self.coord([t % Q for t in self.comps(c)])
        X, Y, ZZ, ZZZ = red(X), red(Y), red(ZZ), red(ZZZ)
        if ZZ == K.zero:
            return None
        return (K.mul(X, K.inv(ZZ)), K.mul(Y, K.inv(ZZZ)))

    def lift(self, P, lam, kx=0, ky=0, kzz=0, kzzz=0):
        """XYZZ values of P with ZZ = lam^2, ZZZ = lam^3, in Montgomery form, each
        coordinate (component-wise for G2) moved to the representative + k p"""
        K = self.K
        l2 = K.mul(lam, lam)
        l3 = K.mul(l2, lam)
        mont = lambda c, k: self.coord([t * RAD % Q + kk * Q for t, kk in
                                        zip(self.comps(c), self.comps(k) if not isinstance(k, int)
                                            else (k,) * len(self.comps(c)))])
        return (mont(K.mul(P[0], l2), kx), mont(K.mul(P[1], l3), ky), mont(l2, kzz), mont(l3, kzzz))


G1 = Group("G1", 0, Fp1, (1, 2))
G2 = Group("G2", 1, Fp2, (
    (10857046999023057135944570762232829481370756359578518086990519993285655852781,
     11559732032986387107991004021392285783925812861821192530917403151452391805634),
    (8495653923123431417604973247489272438418190587263600148770280649306958101930,
     4082367875863433681332203403145435568316851327593401208105741076214120093531)))
GROUPS = (G1, G2)


def curve_ops_of(G):
    return [op for op in CURVE_OPS if not (op.endswith("_g1") or op.endswith("_g1f")) or G is G1
            if not op.endswith("_g2") or G is G2]


# op -> (P is affine, Q: None / "aff" / "xyzz", P may be infinity, Q may be infinity, kmax of P.x)
_SHAPE = {
    "xyzz_madd_g1": (False, "aff", True, False, 8), "xyzz_madd_g1f": (False, "aff", False, False, 8),
    "xyzz_mmadd_g1": (True, "aff", False, False, 2), "xyzz_add_g1": (False, "xyzz", True, True, 2),
    "xyzz_madd_g2": (False, "aff", True, False, 2), "xyzz_mmadd_g2": (True, "aff", False, False, 2),
    "xyzz_add_g2": (False, "xyzz", True, True, 2), "xyzz_mdbl": (True, None, False, False, 2),
    "xyzz_dbl": (False, None, True, False, 2), "xyzz_madd": (False, "aff", True, False, 2),
    "xyzz_add": (False, "xyzz", True, True, 2),
}
X_BOUND = {"xyzz_madd_g1": 8, "xyzz_madd_g1f": 8, "xyzz_mmadd_g1": 8}  # Out: x < 8p; everything else < 2p


class CurveCases(Cases):
    pass


def curve_cases(op, G):
    """Cases for a curve op, with want[i] the model's affine sum (None: infinity)
    and for xyzz_madd_g1f the expected *inf in wflag[i]."""
    K = G.K
    p_aff, q_kind, p_inf_ok, q_inf_ok, kx_max = _SHAPE[op]
    rng = np.random.default_rng(SEED + 100 + CURVE_OPS.index(op) + 50 * G.id)
    rnd = lambda: G.coord([_rand_below(rng, Q - 1) + 1 for _ in G.comps(K.one)])
    pts = [G.mul(k) for k in (1, 2, 3, 5, 0x1234567, R - 1, _rand_below(rng, R))]
    ncomp = len(G.comps(K.one))
    zero_c = G.coord([0] * ncomp)

    def limbs(c):
        return tuple(l for t in G.comps(c) for l in norm(t))

    def ks(kmax):
        """the representative shifts of one coordinate: every k below kmax, per component"""
        if ncomp == 1:
            return list(range(1, kmax))
        return [(k, 0) for k in range(1, kmax)] + [(0, k) for k in range(1, kmax)]

    scen = [(pts[0], pts[1]), (pts[2], pts[4]), (pts[6], pts[3]), (pts[5], pts[0]),   # generic ((r-1)G + G = inf)
            (pts[1], pts[1]), (pts[4], pts[4]), (pts[6], pts[6]),                     # Q = P -> 2P
            (pts[1], G.neg(pts[1])), (pts[4], G.neg(pts[4])), (pts[6], G.neg(pts[6]))]  # Q = -P -> infinity
    if q_kind is None:
        scen = [(P, None) for P in pts]
    rows, flags, what, want, wflag = [], [], [], [], []

    def put(prow, qrow, P, S, note):
        rows.append(list(prow) + [limbs(zero_c)] * (4 - len(prow)) + list(qrow))
        flags.append(0xA5A5A5A5 if op == "xyzz_madd_g1f" else 0)
        W = G.add(P, P) if q_kind is None else G.add(P, S)
        want.append(W)
        wflag.append(int(W is None))
        what.append(note)

    np_, nq = (2 if p_aff else 4), {None: 0, "aff": 2, "xyzz": 4}[q_kind]
    top = lambda kmax: (kmax - 1) if ncomp == 1 else (kmax - 1, kmax - 1)
    all_top = {s: top(kx_max if s == 0 else 2) for s in range(np_ + nq)}
    # one coordinate at a time at every representative it may take, then all at their largest
    every = [{}]
    for slot in range(np_ + nq):
        every += [{slot: k} for k in ks(kx_max if slot == 0 else 2)]
    every.append(all_top)

    def emit(tag, P, S, lam_p, lam_q, variants):
        for var in variants:
            kp = [var.get(s, 0) for s in range(np_)]
            kq = [var.get(np_ + s, 0) for s in range(nq)]
            prow = [limbs(c) for c in G.lift(P, lam_p, *kp)[:np_]]
            if q_kind is None:
                put(prow, [], P, None, f"{tag} lam {lam_p} k {var}")
                continue
            qrow = [limbs(c) for c in G.lift(S, lam_q, *kq)[:nq]]
            put(prow, qrow, P, S, f"{tag} lam {lam_p}/{lam_q} k {var}")
            if op == "xyzz_madd_g1f":
                # the affine y as the bucket kernel feeds a negative digit: 2p - y' limb-wise,
                # for y' the negated y and for y' + p
                ny = (-S[1]) % Q * RAD % Q + var.get(np_ + 1, 0) * Q
                by = tuple((c - a) & 0xFFFFFFFF for c, a in zip(borrow_form(FQ, 2, 1), norm(ny)))
                assert val(by) == 2 * Q - ny
                put(prow, [qrow[0], by], P, S, f"{tag} lam {lam_p} k {var} qy = B2_1 - {ny:#x}")

    for si, (P, S) in enumerate(scen):
        for lam_p in ((K.one,) if p_aff else (K.one, rnd())):
            for lam_q in ((K.one, rnd()) if q_kind == "xyzz" else (K.one,)):
                emit(f"scenario {si}", P, S, lam_p, lam_q, every)
    if q_kind is not None:
        # every ordered pair of distinct points under fresh random lam: the intermediate residues
        # (R^2, PPP, Q, X3) land all over [0, p), which is what decides whether a biased
        # difference such as Q - X3 + 8p comes near its ends
        for i, P in enumerate(pts):
            for j, S in enumerate(pts):
                if i != j:
                    for n in range(1 if p_aff else 2):
                        emit(f"pair {i},{j}", P, S, K.one if p_aff else rnd(),
                             rnd() if q_kind == "xyzz" else K.one, ({}, all_top))
    inf4 = [limbs(zero_c)] * 4
    if p_inf_ok:
        for S in pts[:3]:
            for lam_q in ((K.one, rnd()) if q_kind == "xyzz" else (K.one,)):
                if q_kind is None:
                    put(inf4, [], None, None, "P = infinity")
                else:
                    put(inf4, [limbs(c) for c in G.lift(S, lam_q)[:4 if q_kind == "xyzz" else 2]], None, S,
                        "P = infinity")
    if q_inf_ok:
        for P in pts[:3]:
            for lam_p in (K.one, rnd()):
                put([limbs(c) for c in G.lift(P, lam_p, 1, 1, 1, 1)], inf4, P, None, "Q = infinity")
        put(inf4, inf4, None, None, "both infinity")
    c = CurveCases(rows, flags, what, G.width, seed=200 + CURVE_OPS.index(op) + 50 * G.id)
    # Cases shuffled (and padded) rows and what; bring want / wflag along by description
    key = {id(r): i for i, r in enumerate(rows)}
    order = [key[id(r)] for r in c.rows]
    c.want = [want[i] for i in order]
    c.wflag = [wflag[i] for i in order]
    return c


def curve_out(G, row):
    """the four output coordinates of one case as values (ints, or pairs for G2)"""
    row = np.asarray(row).reshape(4, -1, NL)
    return [G.coord([val(c) for c in coord]) for coord in row]


# ---------------------------------------------------- running and checking
def load(name):
    """one of the two op-table libraries that the build leaves beside libzkmi.so"""
    import ctypes
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zelana_amd", name)
    assert os.path.exists(path), f"{name} is not built (zelana_amd/build_native.py builds it)"
    return ctypes.CDLL(path)


def run(fn, sel, op_id, cases, width=NL):
    """cases through an entry of ff_host_shim.cpp / ff_probe.hip: (out (n, 4, width), flag (n,))"""
    import ctypes
    out = np.zeros((cases.n, 4, width), np.uint32)
    flag = cases.flag.copy()
    inp = np.ascontiguousarray(cases.inp)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_int(sel), ctypes.c_int(op_id), P(inp), P(out), P(flag), ctypes.c_int(cases.n))
    assert rc == 0, f"op {op_id}: the library returned {rc}"
    return out, flag


LIMBWISE = ("add_lazy", "bsub_b2_1", "bsub_b4_1", "bsub_b8_1", "bsub_b10_1", "bsub2_b6_3", "bsubadd_b10_1")


def check_field(op, F, cases, out, flag, leg):
    """every lane: the exact limbs of the model, limbs 0..7 normalised (or below
    the limb-wise form's own limit), the value inside the documented range"""
    nout = N_OUT.get(op, 1)
    limb_hi = {"add_lazy": L31, "bsub2_b6_3": L31, "bsubadd_b10_1": L15}.get(op, L30 if op in LIMBWISE else L29)
    for i in range(cases.n):
        x = [tuple(int(l) for l in r) for r in cases.inp[i]]
        fin = int(cases.flag[i])
        want, wflag = field_model(op, F, x, fin)
        got = [tuple(int(l) for l in out[i, j]) for j in range(nout)]
        hi = out_bound(op, F, x, fin)
        for j in range(nout):
            head = f"{leg} {op}<{F}> lane {i} output {j}: operands {cases.what[i]}"
            assert got[j] == want[j], (f"{head}: got - want = {val(got[j]) - val(want[j]):#x}, got limbs "
                                       f"{[hex(l) for l in got[j]]}, want {[hex(l) for l in want[j]]}")
            assert max(got[j][:NL - 1]) < limb_hi, f"{head}: limbs {[hex(l) for l in got[j]]} not below {limb_hi:#x}"
            assert hi is None or val(got[j]) < hi, f"{head}: value {val(got[j]):#x} not below {hi:#x}"
        if wflag is not None:
            assert int(flag[i]) == wflag, f"{leg} {op}<{F}> lane {i}: flag {int(flag[i])}, want {wflag}: {cases.what[i]}"


def check_curve(op, G, cases, out, flag, leg):
    """every lane: to_affine(output) is the model's point, or both are infinity
    (ZZ = ZZZ = 0 exactly, *inf set for xyzz_madd_g1f); every coordinate meets
    the op's "Out:" line"""
    xb = X_BOUND.get(op, 2)
    for i in range(cases.n):
        head = f"{leg} {op} {G} lane {i} ({cases.what[i]})"
        assert int(out[i].reshape(4, -1, NL)[:, :, :NL - 1].max()) <= MASK, f"{head}: limbs not normalised"
        X, Y, ZZ, ZZZ = curve_out(G, out[i])
        for name, c, k in (("x", X, xb), ("y", Y, 2), ("zz", ZZ, 2), ("zzz", ZZZ, 2)):
            assert all(t < k * Q for t in G.comps(c)), f"{head}: {name} = {c} not below {k}p"
        got, want = G.to_affine(X, Y, ZZ, ZZZ), cases.want[i]
        if want is None:
            assert not out[i, 2:].any(), f"{head}: want infinity as ZZ = ZZZ = 0, got zz {ZZ} zzz {ZZZ}"
        else:
            assert got == want, f"{head}: got {got}, want {want}"
            K = G.K  # ZZ^3 = ZZZ^2 (on Montgomery values: one factor R apart)
            assert K.mul(K.mul(ZZ, ZZ), ZZ) == K.scale(K.mul(ZZZ, ZZZ), RAD % Q), f"{head}: ZZ^3 != ZZZ^2"
        if op == "xyzz_madd_g1f":
            assert int(flag[i]) == cases.wflag[i], f"{head}: *inf = {int(flag[i])}, want {cases.wflag[i]}"
