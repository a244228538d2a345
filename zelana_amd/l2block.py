"""L2BlockCircuit: the reference's Groth16 circuit as an R1CS + full assignment.

Restates prover/src/l2_circuit.rs:180-505 (ConstraintSynthesizer for
L2BlockCircuit) together with the arkworks 0.5 gadgets it calls, so that
`Groth16Prover.prove(inputs, witness)` runs the reference's whole flow
(core/src/sequencer/settlement/prover.rs:350-425) with every field/curve/
polynomial operation on the GPU.  Host work here is synthesis only (~6k
constraints for the dummy() shape; the MSMs/NTTs are in libzkmi).

Gadget semantics followed (3P, pinned in Cargo.lock):
  * ark-crypto-primitives 0.5.0  sponge/poseidon: find_poseidon_ark_and_mds
    (Grain LFSR, rejection-sampled round constants, Cauchy MDS 1/(x_i + y_j)),
    PoseidonSponge / PoseidonSpongeVar duplex (state = capacity || rate,
    absorb adds into state[capacity + i], permute when the rate is full or on
    the first squeeze; full rounds / 2, partial, full rounds / 2; S-box x^alpha
    by pow_by_constant -> x^2, x^4, x^5: three constraints per variable S-box).
  * ark-r1cs-std 0.5.0  FpVar: constants fold, linear ops are symbolic LCs
    (inlined: OptimizationGoal::Constraints), var*var allocates the product;
    enforce_equal => (self - other) * 1 = 0 (a constant side first: c - v);
    enforce_cmp(other, Greater, true) => other < self + 1 with both sides
    <= (p-1)/2 (to_non_unique_bits_le + enforce_smaller_or_equal_than_le),
    then bit 0 of 2*(left - right) (to_bits_le, enforce_in_field_le) * 1 = 1.
    Booleans: (1 - b) * b = 0; and: a * b = c; kary_and of > 3 bits via
    is_eq(sum, k) (is_neq: (c - v) * m = ne, (c - v) * (1 - ne) = 0).
  * Variable order: One, the 7 instances, then witnesses in allocation order.

PARITY UNPINNED: no fixture in the reference covers this
R1CS, and arkworks' sources are not in this image, so the gadget internals
above are a restatement of the published crates' algorithms that cannot be
checked byte-for-byte here.  What IS checked: the R1CS is satisfied by honest
witnesses whose public inputs come from the native sponge, the instance count
is 8 (l2_circuit.rs:513-542), and GPU proofs equal the oracle's on the same
matrices/z/r/s (tests/test_l2block.py, tests/test_gpu_l2block.py).
"""
from __future__ import annotations

from dataclasses import dataclass, field

from .r1cs import R1CS, R

MODULUS_BITS = 254
HALF = (R - 1) // 2


# =================================================================== Poseidon
class GrainLFSR:
    """PoseidonGrainLFSR (ark-crypto-primitives 0.5.0 sponge/poseidon/grain_lfsr.rs)."""

    def __init__(self, prime_bits, state_len, full_rounds, partial_rounds, sbox_inverse=False):
        s = [False] * 80
        s[1] = True  # b0 b1 = 01: prime field
        s[5] = bool(sbox_inverse)  # b2..b5: S-box
        for lo, hi, val in ((6, 17, prime_bits), (18, 29, state_len), (30, 39, full_rounds), (40, 49, partial_rounds)):
            for i in range(hi, lo - 1, -1):
                s[i] = bool(val & 1)
                val >>= 1
        for i in range(50, 80):
            s[i] = True
        self.s, self.head, self.bits = s, 0, prime_bits
        for _ in range(160):
            self._update()

    def _update(self):
        s, h = self.s, self.head
        b = s[(h + 62) % 80] ^ s[(h + 51) % 80] ^ s[(h + 38) % 80] ^ s[(h + 23) % 80] ^ s[(h + 13) % 80] ^ s[h]
        s[h] = b
        self.head = (h + 1) % 80
        return b

    def get_bits(self, n):
        out = []
        for _ in range(n):
            b = self._update()
            while not b:
                self._update()
                b = self._update()
            out.append(self._update())
        return out

    def _int_msb_first(self):
        v = 0
        for b in self.get_bits(self.bits):
            v = (v << 1) | int(b)
        return v

    def field_elements_rejection(self, k):
        out = []
        for _ in range(k):
            while True:
                # F::from_random_bytes keeps the low MODULUS_BITS bits of the
                # sample (ark-ff masks the rest off) before the range check: a
                # no-op for prime_bits = 254, bit 254 dropped for 255
                v = self._int_msb_first() & ((1 << MODULUS_BITS) - 1)
                if v < R:
                    out.append(v)
                    break
        return out

    def field_elements_mod_p(self, k):
        return [self._int_msb_first() % R for _ in range(k)]


_PARAMS = {}


def poseidon_params(rate=2, full_rounds=8, partial_rounds=56, alpha=5, skip_matrices=0, prime_bits=MODULUS_BITS):
    """get_poseidon_config() (l2_circuit.rs:68-83): find_poseidon_ark_and_mds
    (254, rate 2, 8 full, 56 partial, skip 0), capacity 1, alpha 5.
    prime_bits is find_poseidon_ark_and_mds' first argument (the Grain LFSR's
    sample width; circuit/shielded.rs:366 passes 255)."""
    key = (rate, full_rounds, partial_rounds, alpha, skip_matrices, prime_bits)
    if key not in _PARAMS:
        t = rate + 1
        lfsr = GrainLFSR(prime_bits, t, full_rounds, partial_rounds)
        ark = [lfsr.field_elements_rejection(t) for _ in range(full_rounds + partial_rounds)]
        for _ in range(skip_matrices):
            lfsr.field_elements_mod_p(2 * t)
        xs = lfsr.field_elements_mod_p(t)
        ys = lfsr.field_elements_mod_p(t)
        mds = [[pow((xs[i] + ys[j]) % R, R - 2, R) for j in range(t)] for i in range(t)]
        _PARAMS[key] = dict(ark=ark, mds=mds, rate=rate, capacity=1, full=full_rounds, partial=partial_rounds,
                            alpha=alpha)
    return _PARAMS[key]


# ============================================================ constraint system
class CS:
    """Append-only R1CS in arkworks allocation order (One = 0, instances, witnesses)."""

    def __init__(self):
        self.inst = [1]
        self.wit = []
        self.rows = []  # (a, b, c) as {symbol: coeff}; symbols ('i', k) / ('w', k)

    def new_input(self, v):
        self.inst.append(v % R)
        return {("i", len(self.inst) - 1): 1}

    def new_witness(self, v):
        self.wit.append(v % R)
        return {("w", len(self.wit) - 1): 1}

    def enforce(self, a, b, c):
        self.rows.append((a, b, c))

    def to_r1cs(self):
        ni = len(self.inst)

        def idx(sym):
            return sym[1] if sym[0] == "i" else ni + sym[1]

        cs = R1CS(num_instance=ni, num_witness=len(self.wit))
        for a, b, c in self.rows:
            cs.enforce(*[[(idx(s), k) for s, k in lc.items() if k] for lc in (a, b, c)])
        return cs, self.inst + self.wit


ONE = ("i", 0)


def _lc_add(a, b, s=1):
    out = dict(a)
    for k, v in b.items():
        out[k] = (out.get(k, 0) + s * v) % R
    return out


def _lc_scale(a, c):
    return {k: v * c % R for k, v in a.items()}


class FpVar:
    """FpVar<Fr>: Constant(value) or Var(linear combination, value)."""
    __slots__ = ("cs", "lc", "v")

    def __init__(self, cs, lc, v):
        self.cs, self.lc, self.v = cs, lc, v % R  # lc None => constant

    @property
    def const(self):
        return self.lc is None

    def term(self):  # LC including the constant
        return {ONE: self.v} if self.lc is None else self.lc

    @staticmethod
    def constant(cs, v):
        return FpVar(cs, None, v)

    @staticmethod
    def input(cs, v):
        return FpVar(cs, cs.new_input(v), v)

    @staticmethod
    def witness(cs, v):
        return FpVar(cs, cs.new_witness(v), v)

    def __add__(self, o):
        o = o if isinstance(o, FpVar) else FpVar(self.cs, None, o)
        if self.const and o.const:
            return FpVar(self.cs, None, self.v + o.v)
        return FpVar(self.cs, _lc_add(self.term(), o.term()), self.v + o.v)

    def __sub__(self, o):
        o = o if isinstance(o, FpVar) else FpVar(self.cs, None, o)
        if self.const and o.const:
            return FpVar(self.cs, None, self.v - o.v)
        return FpVar(self.cs, _lc_add(self.term(), o.term(), R - 1), self.v - o.v)

    def scale(self, c):
        if self.const:
            return FpVar(self.cs, None, self.v * c)
        return FpVar(self.cs, _lc_scale(self.lc, c), self.v * c)

    def mul(self, o):
        if self.const:
            return o.scale(self.v)
        if o.const:
            return self.scale(o.v)
        p = FpVar.witness(self.cs, self.v * o.v)
        self.cs.enforce(self.lc, o.lc, p.lc)
        return p

    def square(self):
        if self.const:
            return FpVar(self.cs, None, self.v * self.v)
        p = FpVar.witness(self.cs, self.v * self.v)
        self.cs.enforce(self.lc, self.lc, p.lc)
        return p

    def pow_by_constant(self, e):
        """FieldVar::pow_by_constant: square-and-multiply from res = 1."""
        res = FpVar(self.cs, None, 1)
        for bit in bin(e)[2:]:
            res = res.square()
            if bit == "1":
                res = res.mul(self)
        return res

    @staticmethod
    def conditionally_select(cond: "Boolean", t: "FpVar", f: "FpVar") -> "FpVar":
        """CondSelectGadget for FpVar (ark-r1cs-std 0.5 fields/fp/mod.rs): a
        constant condition picks; two constants give the linear combination
        cond t + (1 - cond) f; otherwise AllocatedFp::conditionally_select: the
        result is a new witness with cond * (t - f) = result - f."""
        cs = cond.cs
        if cond.const:
            return t if cond.v else f
        if t.const and f.const:
            return FpVar(cs, _lc_add(_lc_scale(cond.lc, t.v), _lc_scale(cond.negate().term(), f.v)),
                         t.v if cond.v else f.v)
        res = FpVar.witness(cs, t.v if cond.v else f.v)
        cs.enforce(cond.lc, _lc_add(t.term(), f.term(), R - 1), _lc_add(res.lc, f.term(), R - 1))
        return res

    def enforce_equal(self, o):
        """EqGadget::enforce_equal (conditional on TRUE): (x - y) * 1 = 0, with
        a constant operand lifted first: (c - v) * 1 = 0."""
        if self.const and o.const:
            if self.v != o.v:
                raise ValueError("enforce_equal on unequal constants")
            return
        x, y = (self, o) if not (o.const and not self.const) else (o, self)
        self.cs.enforce(_lc_add(x.term(), y.term(), R - 1), {ONE: 1}, {})

    # ----- bits / comparison (ark-r1cs-std 0.5 fields/fp/cmp.rs, bits)
    def to_non_unique_bits_le(self):
        bits = [Boolean.witness(self.cs, (self.v >> i) & 1) for i in range(MODULUS_BITS)]
        packed = {}
        coeff = 1
        for b in bits:
            packed = _lc_add(packed, _lc_scale(b.lc, coeff))
            coeff = coeff * 2 % R
        self.cs.enforce({}, {}, _lc_add(packed, self.term(), R - 1))
        return bits

    def to_bits_le(self):
        bits = self.to_non_unique_bits_le()
        Boolean.enforce_smaller_or_equal_than_le(bits, R - 1)  # enforce_in_field_le
        return bits

    def enforce_smaller_or_equal_than_mod_minus_one_div_two(self):
        Boolean.enforce_smaller_or_equal_than_le(self.to_non_unique_bits_le(), HALF)

    def enforce_cmp(self, other, greater: bool, or_equal: bool):
        left, right = (other, self) if greater else (self, other)
        if or_equal:
            right = right + 1
        left.enforce_smaller_or_equal_than_mod_minus_one_div_two()
        right.enforce_smaller_or_equal_than_mod_minus_one_div_two()
        is_smaller = (left - right).scale(2).to_bits_le()[0]
        self.cs.enforce(is_smaller.term(), {ONE: 1}, {ONE: 1})

    def is_neq_const(self, c):
        """FpVar::is_neq(Var v, Constant c) -> AllocatedFp(c).is_neq(v)."""
        d = (c - self.v) % R
        ne = Boolean(self.cs, self.cs.new_witness(int(d != 0)), int(d != 0))
        mult = FpVar.witness(self.cs, pow(d, R - 2, R) if d else 1)
        diff = _lc_add({ONE: c % R}, self.term(), R - 1)
        self.cs.enforce(diff, mult.lc, ne.lc)
        self.cs.enforce(diff, ne.negate().term(), {})
        return ne


class Boolean:
    """Boolean<Fr>: Constant(bool) or Var(linear combination, value)."""
    __slots__ = ("cs", "lc", "v")

    def __init__(self, cs, lc, v):
        self.cs, self.lc, self.v = cs, lc, int(v)

    @property
    def const(self):
        return self.lc is None

    def term(self):
        return ({ONE: 1} if self.v else {}) if self.lc is None else self.lc

    @staticmethod
    def witness(cs, v):
        lc = cs.new_witness(v)
        cs.enforce(_lc_add({ONE: 1}, lc, R - 1), lc, {})  # (1 - b) * b = 0
        return Boolean(cs, lc, v)

    def negate(self):
        if self.const:
            return Boolean(self.cs, None, 1 - self.v)
        return Boolean(self.cs, _lc_add({ONE: 1}, self.lc, R - 1), 1 - self.v)

    def and_(self, o):
        if self.const:
            return o if self.v else self
        if o.const:
            return self if o.v else o
        res = Boolean(self.cs, self.cs.new_witness(self.v & o.v), self.v & o.v)
        self.cs.enforce(self.lc, o.lc, res.lc)
        return res

    def enforce_equal_const(self, value: bool):
        if self.const:
            if self.v != int(value):
                raise ValueError("unsatisfiable constant boolean equality")
            return
        diff = _lc_add({ONE: 1}, self.lc, R - 1) if value else self.lc
        self.cs.enforce(diff, {ONE: 1}, {})

    @staticmethod
    def kary_and(bits):
        if len(bits) <= 3:
            cur = bits[0]
            for b in bits[1:]:
                cur = cur.and_(b)
            return cur
        cs = next(b.cs for b in bits)
        total = FpVar(cs, None, 0)
        for b in bits:
            total = total + (FpVar(cs, None, b.v) if b.const else FpVar(cs, b.lc, b.v))
        if total.const:
            return Boolean(cs, None, int(total.v == len(bits)))
        return total.is_neq_const(len(bits)).negate()

    @staticmethod
    def enforce_kary_nand(bits):
        r = Boolean.kary_and(bits).negate()
        if r.const:
            if not r.v:
                raise ValueError("kary_nand of all-true constants")
            return
        r.enforce_equal_const(True)

    @staticmethod
    def enforce_smaller_or_equal_than_le(bits, element: int):
        nbits = element.bit_length()
        it = list(reversed(bits))  # big-endian
        pos = 0
        if len(bits) > nbits:
            # or_result = FALSE | b over the excess top bits; FALSE | b = b, and
            # every call here has exactly one excess bit (254-bit values vs (p-1)/2)
            assert len(bits) - nbits == 1, "multi-bit OR chain not needed by this circuit"
            bits[nbits].enforce_equal_const(False)
            pos += 1
        last_run = Boolean(bits[0].cs, None, 1)
        run = []
        for i in range(nbits - 1, -1, -1):
            a = it[pos]
            pos += 1
            if (element >> i) & 1:
                run.append(a)
            else:
                if run:
                    run.append(last_run)
                    last_run = Boolean.kary_and(run)
                    run = []
                Boolean.enforce_kary_nand([last_run, a])
        assert pos == len(it)
        return run


# ============================================================ Poseidon gadget
class PoseidonSpongeVar:
    """PoseidonSpongeVar (duplex sponge over FpVar); values double as the native sponge."""

    def __init__(self, cs, params):
        self.cs, self.p = cs, params
        t = params["rate"] + params["capacity"]
        self.state = [FpVar(cs, None, 0) for _ in range(t)]
        self.mode, self.idx = "absorb", 0

    def _permute(self):
        p, st = self.p, self.state
        half = p["full"] // 2
        for rnd in range(p["full"] + p["partial"]):
            st = [s + c for s, c in zip(st, p["ark"][rnd])]
            if rnd < half or rnd >= half + p["partial"]:
                st = [s.pow_by_constant(p["alpha"]) for s in st]
            else:
                st[0] = st[0].pow_by_constant(p["alpha"])
            new = []
            for i in range(len(st)):
                cur = FpVar(self.cs, None, 0)
                for j, s in enumerate(st):
                    cur = cur + s.scale(p["mds"][i][j])
                new.append(cur)
            st = new
        self.state = st

    def _absorb_internal(self, start, elems):
        rate, cap = self.p["rate"], self.p["capacity"]
        while True:
            if start + len(elems) <= rate:
                for i, e in enumerate(elems):
                    self.state[cap + i + start] = self.state[cap + i + start] + e
                self.mode, self.idx = "absorb", start + len(elems)
                return
            k = rate - start
            for i, e in enumerate(elems[:k]):
                self.state[cap + i + start] = self.state[cap + i + start] + e
            self._permute()
            elems, start = elems[k:], 0

    def absorb(self, elems):
        if not elems:
            return
        if self.mode == "absorb":
            start = self.idx
            if start == self.p["rate"]:
                self._permute()
                start = 0
            self._absorb_internal(start, list(elems))
        else:
            self._permute()
            self._absorb_internal(0, list(elems))

    def squeeze1(self):
        """squeeze_field_elements(1)[0]."""
        cap, rate = self.p["capacity"], self.p["rate"]
        if self.mode == "absorb":
            self._permute()
            start = 0
        else:
            start = self.idx
            if start == rate:
                self._permute()
                start = 0
        out = self.state[cap + start]
        self.mode, self.idx = "squeeze", start + 1
        return out


def poseidon_hash(*xs: int) -> int:
    """Native PoseidonSponge: absorb(xs) then squeeze one element."""
    cs = CS()
    sp = PoseidonSpongeVar(cs, poseidon_params())
    sp.absorb([FpVar(cs, None, x) for x in xs])
    return sp.squeeze1().v


# ================================================================ the circuit
def _fr_le(b: bytes) -> int:
    """Fr::from_le_bytes_mod_order."""
    return int.from_bytes(bytes(b), "little") % R


@dataclass
class TransactionWitness:  # l2_circuit.rs:45-50
    sender_pk: bytes
    recipient_pk: bytes
    amount: int


@dataclass
class WithdrawalWitness:  # l2_circuit.rs:58-62
    recipient: bytes
    amount: int


@dataclass
class L2BlockCircuit:
    """l2_circuit.rs:94-124 (public inputs as 32-byte LE values, batch_id u64)."""
    pre_state_root: bytes = bytes(32)
    post_state_root: bytes = bytes(32)
    pre_shielded_root: bytes = bytes(32)
    post_shielded_root: bytes = bytes(32)
    withdrawal_root: bytes = bytes(32)
    batch_hash: bytes = bytes(32)
    batch_id: int = 0
    transactions: list = field(default_factory=list)
    initial_accounts: dict = field(default_factory=dict)  # pk bytes -> balance (BTreeMap: sorted keys)
    shielded_commitments: list = field(default_factory=list)  # 32-byte commitments
    withdrawals: list = field(default_factory=list)

    @classmethod
    def dummy(cls):
        """L2BlockCircuit::dummy() (l2_circuit.rs:141-166): the keygen shape."""
        return cls(transactions=[TransactionWitness(bytes([1] * 32), bytes([2] * 32), 100)],
                   initial_accounts={bytes([1] * 32): 1000, bytes([2] * 32): 0})

    def generate_constraints(self, cs: CS):
        """ConstraintSynthesizer::generate_constraints (l2_circuit.rs:180-505).
        Returns the circuit's computed values {name: int} (the roots it enforces)."""
        P = poseidon_params()
        pre_state = FpVar.input(cs, _fr_le(self.pre_state_root))
        post_state = FpVar.input(cs, _fr_le(self.post_state_root))
        pre_shielded = FpVar.input(cs, _fr_le(self.pre_shielded_root))
        post_shielded = FpVar.input(cs, _fr_le(self.post_shielded_root))
        wd_root = FpVar.input(cs, _fr_le(self.withdrawal_root))
        batch_hash = FpVar.input(cs, _fr_le(self.batch_hash))
        batch_id = FpVar.input(cs, int(self.batch_id))
        out = {}

        accounts = {}
        for pk in sorted(self.initial_accounts):
            accounts[pk] = FpVar.witness(cs, int(self.initial_accounts[pk]))
        current = dict(accounts)
        for tx in self.transactions:
            amount = FpVar.witness(cs, int(tx.amount))
            if tx.sender_pk not in current:
                raise ValueError("SynthesisError::AssignmentMissing: sender not in initial_accounts")
            sender = current[tx.sender_pk]
            recipient = current.get(tx.recipient_pk, FpVar(cs, None, 0))
            sender.enforce_cmp(amount, greater=True, or_equal=True)
            current[tx.sender_pk] = sender - amount
            current[tx.recipient_pk] = recipient + amount

        def sponge(*elems):
            sp = PoseidonSpongeVar(cs, P)
            sp.absorb(list(elems))
            return sp.squeeze1()

        ds = FpVar.constant(cs, _fr_le(b"zelana:accounts-fold:v1"))

        def fold_accounts(accts):
            st = sponge(ds, batch_id)
            for pk in sorted(accts):
                pk_var = FpVar.witness(cs, _fr_le(pk))
                leaf = sponge(pk_var, accts[pk])
                st = sponge(st, leaf)
            count = FpVar.witness(cs, len(accts))
            return sponge(st, count)

        computed_post = fold_accounts(current)
        out["post_state_root"] = computed_post.v
        computed_post.enforce_equal(post_state)

        sh = sponge(pre_shielded)
        for cm in self.shielded_commitments:
            cm_var = FpVar.witness(cs, _fr_le(cm))
            sh = sponge(sh, cm_var)
        if not self.shielded_commitments:
            out["post_shielded_root"] = pre_shielded.v
            pre_shielded.enforce_equal(post_shielded)
        else:
            out["post_shielded_root"] = sh.v
            sh.enforce_equal(post_shielded)

        wd = sponge(FpVar.constant(cs, _fr_le(b"zelana:withdrawals:v1")))
        for w in self.withdrawals:
            rcp = FpVar.witness(cs, _fr_le(w.recipient))
            amt = FpVar.witness(cs, int(w.amount))
            leaf = sponge(rcp, amt)
            wd = sponge(wd, leaf)
        wd_count = FpVar.witness(cs, len(self.withdrawals))
        computed_wd = sponge(wd, wd_count)
        out["withdrawal_root"] = computed_wd.v
        computed_wd.enforce_equal(wd_root)

        bst = sponge(FpVar.constant(cs, _fr_le(b"zelana:batch-hash:v1")), batch_id)
        for tx in self.transactions:
            s_var = FpVar.witness(cs, _fr_le(tx.sender_pk))
            r_var = FpVar.witness(cs, _fr_le(tx.recipient_pk))
            a_var = FpVar.witness(cs, int(tx.amount))
            txh = sponge(s_var, r_var, a_var)
            bst = sponge(bst, txh)
        tx_count = FpVar.witness(cs, len(self.transactions))
        computed_bh = sponge(bst, tx_count)
        out["batch_hash"] = computed_bh.v
        computed_bh.enforce_equal(batch_hash)

        computed_pre = fold_accounts(accounts)
        out["pre_state_root"] = computed_pre.v
        computed_pre.enforce_equal(pre_state)
        return out

    def synthesize(self):
        """-> (R1CS, full assignment z as ints, computed public values)."""
        cs = CS()
        out = self.generate_constraints(cs)
        r1cs, z = cs.to_r1cs()
        return r1cs, z, out

    def with_consistent_inputs(self):
        """A copy whose public inputs are the values the circuit computes (an
        honest, satisfiable instance; the reference's own prove path feeds
        blake3 batch hashes and so is never satisfied)."""
        _, _, out = self.synthesize()
        enc = {k: v.to_bytes(32, "little") for k, v in out.items()}
        c = L2BlockCircuit(**{**self.__dict__})
        c.pre_state_root = enc["pre_state_root"]
        c.post_state_root = enc["post_state_root"]
        c.post_shielded_root = enc["post_shielded_root"]
        c.withdrawal_root = enc["withdrawal_root"]
        c.batch_hash = enc["batch_hash"]
        return c


def public_inputs_fr(c: L2BlockCircuit) -> list[int]:
    """The 7 instance values in allocation order (what a verifier feeds)."""
    return [_fr_le(c.pre_state_root), _fr_le(c.post_state_root), _fr_le(c.pre_shielded_root),
            _fr_le(c.post_shielded_root), _fr_le(c.withdrawal_root), _fr_le(c.batch_hash), int(c.batch_id) % R]
