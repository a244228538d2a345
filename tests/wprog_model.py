"""One plain-integer model of the witness-program ABI (include/zkmi.h,
"witness programs"), all ten op kinds, and a builder of small programs in
zkmi_wprog_desc layout.

The interpreter is written from the header's op descriptions alone: Python
ints mod r, no Montgomery form, no limbs, no scheduling.  It walks the ops in
array order, which a valid program's levels allow (an op reads inputs and
earlier levels only).  tests/test_wprog_model_cpu.py pins it to the three
interpreters the recorders ship with; tests/test_gpu_wprog_ops.py compares
wprog.hip with it.
"""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

MUL, INV, BITS64, PERM, BITS, NZ, POSEIDON, INV1, POSEIDON_RC, SELECT = range(1, 11)
MIMC_ROUNDS = 91
MIMC_C = [(i + 1) ** 3 + (i + 1) for i in range(MIMC_ROUNDS)]
L2_FULL, L2_PARTIAL = 8, 56  # kind 7's round counts


def limbs(z) -> np.ndarray:
    """ints -> (n, 4) canonical u64 limbs"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in z)
    return np.frombuffer(raw, np.uint64).reshape(-1, 4).copy()


def _ints(rows) -> list:
    rows = np.ascontiguousarray(rows, np.uint64).reshape(-1, 4)
    raw = rows.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(rows.shape[0])]


def rc_word(nterms2: int, mask: int, full: int, partial: int) -> int:
    """word 3 of a kind-9 op"""
    return nterms2 | (mask << 16) | (partial << 19) | ((full // 2) << 27)


def poseidon_len(mask: int, full: int, partial: int) -> int:
    half = full // 2
    return 3 * bin(mask).count("1") + 9 * (half - 1) + 3 * partial + 9 * half


def span(kind: int, w3: int) -> int:
    """number of z values an op writes, from its kind and word 3"""
    if kind == BITS64:
        return 64
    if kind == BITS:
        return w3
    if kind == PERM:
        return 4 * MIMC_ROUNDS
    if kind == POSEIDON:
        return poseidon_len(w3 >> 16, L2_FULL, L2_PARTIAL)
    if kind == POSEIDON_RC:
        return poseidon_len((w3 >> 16) & 7, 2 * (w3 >> 27), (w3 >> 19) & 0xFF)
    return 1


def _poseidon(x, mask, full, partial, coeff):
    """the trace: x^2, x^4, x^5 of every S-box in round order (round 0 only for
    the masked elements)"""
    rounds, half = full + partial, full // 2
    mds = [[coeff[3 * rounds + 3 * i + j] for j in range(3)] for i in range(3)]
    out = []
    for r in range(rounds):
        x = [(x[i] + coeff[3 * r + i]) % R for i in range(3)]
        is_full = r < half or r >= rounds - half
        for i in range(3 if is_full else 1):
            x2 = x[i] * x[i] % R
            x4 = x2 * x2 % R
            x5 = x4 * x[i] % R
            if r > 0 or (mask >> i) & 1:
                out += [x2, x4, x5]
            x[i] = x5
        x = [sum(mds[i][j] * x[j] for j in range(3)) % R for i in range(3)]
    return out


def interpret(prog, inputs) -> list:
    """The full assignment z (ints) of `prog` (anything with num_vars,
    input_var, op, term, coeff in zkmi_wprog_desc layout) over `inputs`
    ((num_inputs, 4) canonical u64)."""
    z = [0] * int(prog.num_vars)
    for var, v in zip(np.asarray(prog.input_var).tolist(), _ints(inputs)):
        z[var] = v
    coeff = _ints(prog.coeff)
    term = np.asarray(prog.term, np.uint32).reshape(-1, 2).tolist()

    def lc(off, n):
        return sum(z[v] * coeff[c] for v, c in term[off:off + n]) % R

    for w0, out, a_off, w3 in np.asarray(prog.op, np.uint32).reshape(-1, 4).tolist():
        kind, a_len, b_len = w0 & 0xFF, (w0 >> 8) & 0xFFF, w0 >> 20
        if kind in (POSEIDON, POSEIDON_RC, SELECT):
            x = [lc(a_off, a_len), lc(a_off + a_len, b_len), lc(a_off + a_len + b_len, w3 & 0xFFFF)]
            if kind == SELECT:
                z[out] = x[1] if x[0] else x[2]
                continue
            if kind == POSEIDON:
                tr = _poseidon(x, w3 >> 16, L2_FULL, L2_PARTIAL, coeff)
            else:
                tr = _poseidon(x, (w3 >> 16) & 7, 2 * (w3 >> 27), (w3 >> 19) & 0xFF, coeff)
            assert len(tr) == span(kind, w3)
            z[out:out + len(tr)] = tr
            continue
        a = lc(a_off, a_len)
        if kind == MUL:
            z[out] = a * lc(w3, b_len) % R
        elif kind == INV:
            z[out] = pow(a, R - 2, R)  # 0 -> 0
        elif kind == INV1:
            z[out] = pow(a, R - 2, R) if a else 1
        elif kind == NZ:
            z[out] = int(a != 0)
        elif kind in (BITS64, BITS):
            for i in range(64 if kind == BITS64 else w3):
                z[out + i] = (a >> i) & 1
        elif kind == PERM:
            t = a
            for r in range(MIMC_ROUNDS):
                t = (t + MIMC_C[r]) % R
                t2 = t * t % R
                t4 = t2 * t2 % R
                t6 = t4 * t2 % R
                t = t6 * t % R
                z[out + 4 * r:out + 4 * r + 4] = [t2, t4, t6, t]
        else:
            raise ValueError(f"op kind {kind}")
    return z


class Program:
    """arrays in zkmi_wprog_desc layout (zelana_amd.wprog.WitnessProgram takes it as its plan)"""

    def __init__(self, num_vars, input_var, op, term, coeff, level_start):
        self.num_vars, self.num_instance = int(num_vars), 1
        self.input_var = np.ascontiguousarray(input_var, np.uint32)
        self.op = np.ascontiguousarray(op, np.uint32).reshape(-1, 4)
        self.term = np.ascontiguousarray(term, np.uint32).reshape(-1, 2)
        self.coeff = np.ascontiguousarray(coeff, np.uint64).reshape(-1, 4)
        self.level_start = np.ascontiguousarray(level_start, np.uint32)
        self.num_levels = self.level_start.size - 1
        self.kinds = self.op[:, 0] & 0xFF

    def level_sizes(self) -> list:
        return np.diff(self.level_start.astype(np.int64)).tolist()


def build(num_vars, input_var, ops, poseidon=None, keep_order=False) -> Program:
    """A Program of ops given as (kind, out, extra, [lc, ...]) or (kind, out,
    extra, [lc, ...], level), with lc = [(z index, coefficient int)].

    lcs: one combination (INV, BITS64, PERM, BITS, NZ, INV1), two (MUL) or
    three (POSEIDON, POSEIDON_RC: the state; SELECT: c, t, f).  extra: the
    width of BITS, the mask of kinds 7 and 9, else 0.
    poseidon = (full, partial, table) with table the 3 (full + partial) + 9
    constants (ark[r][i] at 3r + i, then m[i][j]); it leads the coefficient
    table and the other coefficients are interned after it.
    An op's level is 1 + the deepest level among the variables it reads
    (inputs are level 0) unless it names one, which must still be deeper than
    everything it reads; a level number nobody uses becomes an empty level.
    Within a level permutations (kinds 4, 7, 9) come first, as the recorders
    order them, then the caller's order; keep_order=True keeps the caller's
    order alone."""
    table, ids = [], {}
    full = partial = 0
    if poseidon is not None:
        full, partial, consts = poseidon
        table = [int(c) % R for c in consts]
        assert len(table) == 3 * (full + partial) + 9
    npos = len(table)

    def cid(c):
        c %= R
        i = ids.get(c)
        if i is None:
            i = ids[c] = npos + len(ids)
            table.append(c)
        return i

    level = [-1] * num_vars
    readable = [True] * num_vars  # False: a trace value that stays in Montgomery form until the run's end
    for v in np.asarray(input_var).tolist():
        level[v] = 0
    sched = []
    for n, o in enumerate(ops):
        kind, out, extra, lcs = o[:4]
        assert len(lcs) == (2 if kind == MUL else 3 if kind in (POSEIDON, POSEIDON_RC, SELECT) else 1)
        reads = [v for lc in lcs for v, _ in lc]
        assert all(level[v] >= 0 for v in reads), "op reads a variable nothing has produced"
        assert all(readable[v] for v in reads), "only a permutation's output values may be read"
        lv = 1 + max([level[v] for v in reads] or [0])
        if len(o) > 4:
            assert o[4] >= lv, "level override above the op's inputs"
            lv = o[4]
        if kind == POSEIDON:
            assert (full, partial) == (L2_FULL, L2_PARTIAL)
            w3 = len(lcs[2]) | (extra << 16)
        elif kind == POSEIDON_RC:
            w3 = rc_word(len(lcs[2]), extra, full, partial)
        elif kind == SELECT:
            w3 = len(lcs[2])
        elif kind == BITS:
            w3 = extra
        else:
            w3 = 0  # MUL: b_off, set below
        n_out = span(kind, w3)
        assert all(x < 0 for x in level[out:out + n_out]) and out + n_out <= num_vars, "variable written twice"
        level[out:out + n_out] = [lv] * n_out
        if kind in (POSEIDON, POSEIDON_RC):
            readable[out:out + n_out] = [False] * n_out
            for k in (7, 4, 1):
                readable[out + n_out - k] = True
        elif kind == PERM:
            readable[out:out + n_out - 1] = [False] * (n_out - 1)
        sched.append((lv, 0 if keep_order or kind not in (PERM, POSEIDON, POSEIDON_RC) else -1, n, w3))
    assert all(x >= 0 for x in level), "variables neither inputs nor op outputs"
    sched.sort()
    terms, oparr, lvs = [], np.zeros((len(ops), 4), np.uint32), []
    for i, (lv, _, n, w3) in enumerate(sched):
        kind, out, _, lcs = ops[n][:4]
        off = len(terms)
        lens = []
        for lc in lcs:
            assert len(lc) < 4096
            lens.append(len(lc))
            if kind == MUL and len(lens) == 2:
                w3 = len(terms)
            terms += [(v, cid(c)) for v, c in lc]
        oparr[i] = (kind | (lens[0] << 8) | ((lens[1] if len(lens) > 1 else 0) << 20), out, off, w3)
        lvs.append(lv)
    nlev = max(lvs) if lvs else 0
    level_start = np.searchsorted(np.array(lvs, np.int64), np.arange(1, nlev + 2))
    if not table:
        table.append(1)  # num_coeffs >= 1
    coeff = np.frombuffer(b"".join(c.to_bytes(32, "little") for c in table), np.uint64).reshape(-1, 4)
    term = np.array(terms, np.uint32).reshape(-1, 2) if terms else np.zeros((0, 2), np.uint32)
    return Program(num_vars, input_var, oparr, term, coeff, level_start)
