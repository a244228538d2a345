"""ShieldedTransferCircuit: the reference's shielded-transfer Groth16 circuit
as an R1CS, a full assignment and a GPU witness program, with a batched prover.

Restates prover/src/circuit/shielded.rs:142-368 (ConstraintSynthesizer for
ShieldedTransferCircuit) over l2block.py's gadgets.  Every user transfer makes
one proof of this circuit (18,927 constraints for 2 inputs, 2 outputs and
depth-32 Merkle paths: a 2^15 domain), so it is the workload of the batched
calls: witnesses by zkmi_wprog_run_many, proofs by zkmi_groth16_prove_many,
verification by verify_many / verify_each / the verifiers over wire bytes
(ShieldedProver below).

Circuit (shielded.rs line numbers):
  * public inputs, in this order (:146-170): merkle_root, nullifiers...,
    commitments..., fee; witnesses in allocation order.
  * per input (:180-232): value, randomness, owner_pk, position, spending_key
    are witnesses; commitment = sponge(value, randomness, owner_pk) (:273-285);
    per Merkle level (:341-358) a sibling witness and a Boolean witness,
    left = select(bit, sibling, current), right = select(bit, current,
    sibling), parent = sponge(left, right); root equality (:360); nullifier =
    sponge(0x4e554c4c, spending_key, commitment, position) (:288-309) equal to
    its public input (:223); sponge(b"ZelanaPK" || 0... mod r, spending_key)
    equal to owner_pk (:312-328, :228).
  * per output (:237-261): value, randomness, recipient_pk witnesses, the
    commitment equal to its public input.
  * balance (:265-266): sum of input values = sum of output values + fee.
  * Poseidon (:365-368): find_poseidon_ark_and_mds(255, 2, 8, 57, 0), rate 2,
    capacity 1, alpha 5: not L2BlockCircuit's parameters (254, 56 partial).

Reference quirks, kept as they are:
  * `position` enters the nullifier only; nothing ties it to the path bits.
  * values are not range-checked (the balance holds mod r).
  * the number of inputs and outputs is whatever the vectors hold (MAX_INPUTS,
    MAX_OUTPUTS and TREE_DEPTH are not enforced).
  * zip(merkle_path, path_bits) truncates to the shorter of the two.
  * so a circuit shape, and with it a proving key, is (path length per
    input..., number of outputs): shape_key().  The public vectors must hold
    one nullifier per input (fewer panic in the reference at :223) and one
    commitment per output; this module refuses other lengths.

PARITY UNPINNED: no fixture in the reference covers this
R1CS (its own test, shielded.rs:370-410, is a placeholder that asserts
nothing), and arkworks' sources are not in this image, so the gadget internals
are a restatement of the published crates' algorithms that cannot be checked
byte-for-byte here.  What IS checked: the R1CS is satisfied by honest
transfers whose public inputs come from the native sponge and unsatisfied, at
the row of the broken equality, by tampered ones; the instance count is 3 +
inputs + outputs; the row count equals the closed form; the recorded witness
program reproduces the synthesis assignment; and GPU proofs equal the oracle's
on the same matrices/z/r/s (tests/test_shielded_cpu.py,
tests/test_gpu_shielded.py).

Witness program: a recording constraint system (RecordingCS) writes the
program while synthesizing: one POSEIDON_RC op (kind 9, zkmi.h) per
permutation, one SELECT op (kind 10) per conditionally_select; the free
inputs (One, the public inputs and the witnesses the circuit allocates
itself) are the program's inputs.  No other op kind is needed: every other
witness is a permutation's trace or a select's result.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from .l2block import CS, Boolean, FpVar, PoseidonSpongeVar, _fr_le, poseidon_params
from .r1cs import R
from .wprog import ProgramArrays

KIND_POSEIDON_RC, KIND_SELECT = 9, 10
NULLIFIER_DOMAIN = 0x4E554C4C  # "NULL" (shielded.rs:298)
PK_DOMAIN = _fr_le(b"ZelanaPK" + bytes(24))  # shielded.rs:320-322


def shielded_params():
    """get_poseidon_config() (shielded.rs:365-368)."""
    return poseidon_params(rate=2, full_rounds=8, partial_rounds=57, alpha=5, skip_matrices=0, prime_bits=255)


def permutation_rows(mask: int, params=None) -> int:
    """Constraints (= trace values) of one permutation whose round-0 state has
    the variables `mask`: three per variable S-box."""
    p = params or shielded_params()
    half = p["full"] // 2
    return 3 * bin(mask).count("1") + 9 * (half - 1) + 3 * p["partial"] + 9 * half


def expected_rows(shape) -> int:
    """Closed-form row count of a shape (path length per input..., n_out)."""
    *depths, n_out = shape
    r6, r7, r4 = permutation_rows(6), permutation_rows(7), permutation_rows(4)
    per_in = sum((r6 + r7) + d * r6 + (r4 + r7) + r4 + 2 * d + d + 3 for d in depths)
    return per_in + n_out * (r6 + r7 + 1) + 1


# ============================================================= native values
def _b32(v: int) -> bytes:
    return (v % R).to_bytes(32, "little")


def _fr(b) -> int:
    return b % R if isinstance(b, int) else _fr_le(b)


def sponge_hash(*xs: int) -> int:
    """Native PoseidonSponge with the shielded parameters: absorb, squeeze one."""
    cs = CS()
    sp = PoseidonSpongeVar(cs, shielded_params())
    sp.absorb([FpVar(cs, None, x) for x in xs])
    return sp.squeeze1().v


def note_commitment(value: int, randomness, owner_pk) -> int:
    return sponge_hash(int(value), _fr(randomness), _fr(owner_pk))


def nullifier(spending_key, commitment, position: int) -> int:
    return sponge_hash(NULLIFIER_DOMAIN, _fr(spending_key), _fr(commitment), int(position))


def derive_pk(spending_key) -> int:
    return sponge_hash(PK_DOMAIN, _fr(spending_key))


def merkle_root(leaf, path, bits) -> int:
    cur = _fr(leaf)
    for sib, right in zip(path, bits):
        s = _fr(sib)
        cur = sponge_hash(s, cur) if right else sponge_hash(cur, s)
    return cur


class NoteTree:
    """A sparse commitment tree of the circuit's hash (empty leaves are 0):
    paths for several leaves under one root."""

    def __init__(self, depth: int):
        self.depth = depth
        self.empty = [0]
        for _ in range(depth):
            self.empty.append(sponge_hash(self.empty[-1], self.empty[-1]))
        self.nodes: dict = {}

    def _get(self, level, idx):
        return self.nodes.get((level, idx), self.empty[level])

    def insert(self, position: int, leaf):
        assert 0 <= position < 1 << self.depth
        self.nodes[(0, position)] = _fr(leaf)
        idx = position
        for level in range(self.depth):
            idx >>= 1
            self.nodes[(level + 1, idx)] = sponge_hash(self._get(level, 2 * idx), self._get(level, 2 * idx + 1))

    def root(self) -> int:
        return self._get(self.depth, 0)

    def path(self, position: int):
        """(sibling bytes per level, is-right bit per level) from the leaf up."""
        sibs, bits = [], []
        idx = position
        for level in range(self.depth):
            sibs.append(_b32(self._get(level, idx ^ 1)))
            bits.append(bool(idx & 1))
            idx >>= 1
        return sibs, bits

    def spend_notes(self, specs) -> list:
        """specs: (value, randomness, spending_key, position) per note.  Inserts
        every note's commitment, then returns the InputNotes with their paths
        under the one resulting root."""
        notes = []
        for value, rand, sk, pos in specs:
            pk = _b32(derive_pk(sk))
            self.insert(pos, note_commitment(value, rand, pk))
            notes.append(InputNote(value, bytes(rand), pk, pos, bytes(sk)))
        for n in notes:
            n.merkle_path, n.path_bits = self.path(n.position)
        return notes


# ================================================= batched hashes, device tree
# The same hashes, domain constants and argument orders as above, n at a time
# on the GPU (gpu.PoseidonHasher: one lane per hash), and the reference's
# MerkleTree / RootHistory (sdk/privacy/src/merkle.rs) over a tree that lives in
# HBM (gpu.NoteTreeDevice).  The functions above stay as they
# are: they are what these are tested against.
ROOT_HISTORY_SIZE = 100  # core/src/sequencer/storage/shielded_state.rs:24


def shielded_hasher(ctx):
    """A gpu.PoseidonHasher over shielded_params()."""
    from . import gpu
    return gpu.PoseidonHasher(ctx, shielded_params())


def _hash_ints(h, tuples) -> list:
    tuples = list(tuples)
    if not tuples:
        return []
    return [_int4(row) for row in h.hash_many(tuples)]


def commit_many(h, notes) -> list:
    """note_commitment of every (value, randomness, owner_pk), one call."""
    return _hash_ints(h, [(int(v) % R, _fr(rand), _fr(pk)) for v, rand, pk in notes])


def nullifier_many(h, spending_keys, commitments, positions) -> list:
    """nullifier(spending_key, commitment, position) element by element, one call."""
    return _hash_ints(h, [(NULLIFIER_DOMAIN, _fr(sk), _fr(cm), int(pos) % R)
                          for sk, cm, pos in zip(spending_keys, commitments, positions)])


def derive_pk_many(h, keys) -> list:
    """derive_pk of every spending key, one call."""
    return _hash_ints(h, [(PK_DOMAIN, _fr(sk)) for sk in keys])


def merkle_root_many(h, leaves, paths, bits_list) -> list:
    """merkle_root of every (leaf, path, bits), one hash_many call per level."""
    cur = [_fr(leaf) for leaf in leaves]
    steps = [list(zip(p, b)) for p, b in zip(paths, bits_list)]
    for level in range(max((len(s) for s in steps), default=0)):
        live = [i for i, s in enumerate(steps) if level < len(s)]
        pairs = []
        for i in live:
            sib, right = steps[i][level]
            pairs.append((_fr(sib), cur[i]) if right else (cur[i], _fr(sib)))
        for i, v in zip(live, _hash_ints(h, pairs)):
            cur[i] = v
    return cur


class DeviceNoteTree:
    """The note commitment tree resident on the GPU, with the reference's root
    history.  empty_leaf=None is the reference's H(0) (a one-element absorb,
    merkle.rs:126-134); empty_leaf=0 reproduces NoteTree.  Append-only: leaves
    take the positions next_position, next_position + 1, ..."""

    def __init__(self, ctx, depth: int = 32, capacity: int = 1 << 20, empty_leaf=None, hasher=None):
        from collections import deque

        from . import gpu
        self.ctx, self.depth = ctx, depth
        self.hasher = hasher or shielded_hasher(ctx)
        if empty_leaf is None:
            empty_leaf = _hash_ints(self.hasher, [(0,)])[0]
        self.dev = gpu.NoteTreeDevice(ctx, self.hasher, depth, capacity, _fr(empty_leaf))
        self.history = deque([self.root()], maxlen=ROOT_HISTORY_SIZE)  # newest last

    @property
    def next_position(self) -> int:
        return self.dev.next_position

    def append(self, leaves):
        """-> (first position, the root after every single insertion as ints);
        each of those roots enters the history, as n inserts would have put it."""
        first, roots = self.dev.append([_fr(v) for v in leaves])
        roots = [_int4(r) for r in roots]
        self.history.extend(roots)
        return first, roots

    def root(self) -> int:
        return _int4(self.dev.root())

    def is_valid_root(self, root) -> bool:
        """RootHistory::is_valid: the current root or one of the last ROOT_HISTORY_SIZE."""
        return _fr(root) in self.history

    def get(self, position: int) -> int:
        return _int4(self.dev.leaves(position, 1)[0])

    def paths(self, positions) -> list:
        """[(sibling bytes per level, is-right bit per level)] as NoteTree.path."""
        positions = [int(p) for p in positions]
        sib = self.dev.paths(positions)
        return [([row.tobytes() for row in sib[i]], [bool((p >> level) & 1) for level in range(self.depth)])
                for i, p in enumerate(positions)]

    def path(self, position: int):
        return self.paths([position])[0]

    def spend_notes(self, specs) -> list:
        """NoteTree.spend_notes: specs are (value, randomness, spending_key,
        position) per note; the positions must be the next free ones, in order."""
        specs = list(specs)
        first = self.next_position
        if [int(s[3]) for s in specs] != list(range(first, first + len(specs))):
            raise ValueError(f"spend_notes: an append-only tree takes positions {first}.. in order")
        pks = [_b32(v) for v in derive_pk_many(self.hasher, [s[2] for s in specs])]
        self.append(commit_many(self.hasher, [(v, rand, pk) for (v, rand, _, _), pk in zip(specs, pks)]))
        notes = [InputNote(v, bytes(rand), pk, pos, bytes(sk)) for (v, rand, sk, pos), pk in zip(specs, pks)]
        for n, (sibs, bits) in zip(notes, self.paths([n.position for n in notes])):
            n.merkle_path, n.path_bits = sibs, bits
        return notes

    def close(self):
        self.dev.close()


def honest_many(h, inputs_list, outputs_list, fees=None, tree=None) -> list:
    """The ShieldedTransfers that ShieldedTransfer.honest(inputs, outputs, fee)
    builds, for many transfers: every nullifier and commitment from one batched
    hash each; the root is `tree`'s when one is given, else the first input's
    path folded on the device."""
    inputs_list = [list(x) for x in inputs_list]
    outputs_list = [list(x) for x in outputs_list]
    fees = [None] * len(inputs_list) if fees is None else list(fees)
    if not len(inputs_list) == len(outputs_list) == len(fees):
        raise ValueError("honest_many: one input list, output list and fee per transfer")
    flat_in = [n for ins in inputs_list for n in ins]
    flat_out = [o for outs in outputs_list for o in outs]
    cms = commit_many(h, [(n.value, n.randomness, n.owner_pk) for n in flat_in])
    nfs = nullifier_many(h, [n.spending_key for n in flat_in], cms, [n.position for n in flat_in])
    out_cms = commit_many(h, [(o.value, o.randomness, o.recipient_pk) for o in flat_out])
    at, firsts = 0, []
    for ins in inputs_list:
        firsts.append(at if ins else None)
        at += len(ins)
    if tree is not None:
        current = tree.root()
        roots = [0 if k is None else current for k in firsts]
    else:
        have = [k for k in firsts if k is not None]
        folded = iter(merkle_root_many(h, [cms[k] for k in have], [flat_in[k].merkle_path for k in have],
                                       [flat_in[k].path_bits for k in have]))
        roots = [0 if k is None else next(folded) for k in firsts]
    res, ai, ao = [], 0, 0
    for ins, outs, fee, root in zip(inputs_list, outputs_list, fees, roots):
        if fee is None:
            fee = sum(n.value for n in ins) - sum(o.value for o in outs)
        res.append(ShieldedTransfer(_b32(root), [_b32(v) for v in nfs[ai:ai + len(ins)]],
                                    [_b32(v) for v in out_cms[ao:ao + len(outs)]], int(fee), ins, outs))
        ai += len(ins)
        ao += len(outs)
    return res


# ================================================================ the circuit
@dataclass
class InputNote:  # shielded.rs:44-59 (InputNoteWitness)
    value: int
    randomness: bytes
    owner_pk: bytes
    position: int
    spending_key: bytes
    merkle_path: list = field(default_factory=list)
    path_bits: list = field(default_factory=list)


@dataclass
class OutputNote:  # shielded.rs:63-70 (OutputNoteWitness)
    value: int
    randomness: bytes
    recipient_pk: bytes


class RecordingCS(CS):
    """CS that also writes the witness program: `free` are the witnesses the
    circuit allocates from its own inputs, `ops` the permutations and selects
    in synthesis order."""

    def __init__(self):
        super().__init__()
        self.free = []  # witness indices that are program inputs
        self.ops = []   # (kind, first witness index, mask, [lc, lc, lc])


class _Sponge(PoseidonSpongeVar):
    """PoseidonSpongeVar whose permutations are recorded as kind-9 ops: state
    in = the three state combinations before round 0, out = the S-box
    witnesses the permutation allocates (x^2, x^4, x^5 in round order)."""

    def _permute(self):
        cs, st_in = self.cs, list(self.state)
        w0 = len(cs.wit)
        super()._permute()
        if isinstance(cs, RecordingCS):
            mask = sum(1 << i for i, s in enumerate(st_in) if not s.const)
            assert mask and len(cs.wit) - w0 == permutation_rows(mask, self.p)
            cs.ops.append((KIND_POSEIDON_RC, w0, mask, [s.term() for s in st_in]))


def _select(cond: Boolean, t: FpVar, f: FpVar) -> FpVar:
    cs = cond.cs
    w0 = len(cs.wit)
    res = FpVar.conditionally_select(cond, t, f)
    if isinstance(cs, RecordingCS) and len(cs.wit) > w0:
        cs.ops.append((KIND_SELECT, w0, 0, [cond.term(), t.term(), f.term()]))
    return res


@dataclass
class ShieldedTransfer:
    """shielded.rs:74-93 (public inputs as 32-byte LE values, fee u64)."""
    merkle_root: bytes = bytes(32)
    nullifiers: list = field(default_factory=list)
    commitments: list = field(default_factory=list)
    fee: int = 0
    inputs: list = field(default_factory=list)
    outputs: list = field(default_factory=list)

    @classmethod
    def dummy(cls, shape):
        """An all-zero transfer of a shape (path length per input..., n_out):
        the keygen instance (the matrices depend on the shape alone)."""
        *depths, n_out = shape
        z = bytes(32)
        return cls(z, [z] * len(depths), [z] * n_out, 0,
                   [InputNote(0, z, z, 0, z, [z] * d, [False] * d) for d in depths],
                   [OutputNote(0, z, z) for _ in range(n_out)])

    @classmethod
    def honest(cls, inputs, outputs, fee=None):
        """The transfer whose public inputs are the values the circuit computes
        for these notes: root of the first input's path, every nullifier and
        commitment, fee = sum in - sum out unless given."""
        inputs, outputs = list(inputs), list(outputs)
        cms = [note_commitment(n.value, n.randomness, n.owner_pk) for n in inputs]
        root = merkle_root(cms[0], inputs[0].merkle_path, inputs[0].path_bits) if inputs else 0
        if fee is None:
            fee = sum(n.value for n in inputs) - sum(o.value for o in outputs)
        return cls(_b32(root), [_b32(nullifier(n.spending_key, cm, n.position)) for n, cm in zip(inputs, cms)],
                   [_b32(note_commitment(o.value, o.randomness, o.recipient_pk)) for o in outputs], int(fee),
                   inputs, outputs)

    def generate_constraints(self, cs: CS):
        """ConstraintSynthesizer::generate_constraints (shielded.rs:143-269).
        Returns the rows of the equalities it enforces: {"root": [row per
        input], "nullifier": [...], "pk": [...], "commitment": [row per
        output], "balance": row}."""
        P = shielded_params()
        if len(self.nullifiers) < len(self.inputs) or len(self.commitments) < len(self.outputs):
            raise ValueError("fewer public nullifiers / commitments than notes (index panic at shielded.rs:223/257)")
        root_var = FpVar.input(cs, _fr_le(self.merkle_root))  # :147-150
        nf_vars = [FpVar.input(cs, _fr_le(nf)) for nf in self.nullifiers]  # :153-158
        cm_vars = [FpVar.input(cs, _fr_le(cm)) for cm in self.commitments]  # :161-166
        fee_var = FpVar.input(cs, int(self.fee))  # :169-170
        rec = isinstance(cs, RecordingCS)

        def witness(v):
            if rec:
                cs.free.append(len(cs.wit))
            return FpVar.witness(cs, v)

        def sponge(*elems):
            sp = _Sponge(cs, P)
            sp.absorb(list(elems))
            return sp.squeeze1()

        rows = {"root": [], "nullifier": [], "pk": [], "commitment": [], "balance": None}
        total_in = FpVar.constant(cs, 0)
        for i, note in enumerate(self.inputs):  # :180-232
            value = witness(int(note.value))
            randomness = witness(_fr_le(note.randomness))
            owner_pk = witness(_fr_le(note.owner_pk))
            position = witness(int(note.position))
            sk = witness(_fr_le(note.spending_key))
            commitment = sponge(value, randomness, owner_pk)  # :195-201, :273-285
            current = commitment  # verify_merkle_path, :331-362
            for sib_bytes, is_right in zip(note.merkle_path, note.path_bits):
                sibling = witness(_fr_le(sib_bytes))
                if rec:
                    cs.free.append(len(cs.wit))
                bit = Boolean.witness(cs, int(bool(is_right)))
                left = _select(bit, sibling, current)
                right = _select(bit, current, sibling)
                current = sponge(left, right)
            rows["root"].append(len(cs.rows))
            current.enforce_equal(root_var)
            nf = sponge(FpVar.constant(cs, NULLIFIER_DOMAIN), sk, commitment, position)  # :288-309
            rows["nullifier"].append(len(cs.rows))
            nf.enforce_equal(nf_vars[i])
            derived = sponge(FpVar.constant(cs, PK_DOMAIN), sk)  # :312-328
            rows["pk"].append(len(cs.rows))
            derived.enforce_equal(owner_pk)
            total_in = total_in + value
        total_out = FpVar.constant(cs, 0)
        for i, note in enumerate(self.outputs):  # :237-261
            value = witness(int(note.value))
            randomness = witness(_fr_le(note.randomness))
            recipient = witness(_fr_le(note.recipient_pk))
            commitment = sponge(value, randomness, recipient)
            rows["commitment"].append(len(cs.rows))
            commitment.enforce_equal(cm_vars[i])
            total_out = total_out + value
        rows["balance"] = len(cs.rows)
        total_in.enforce_equal(total_out + fee_var)  # :265-266
        return rows

    def synthesize(self):
        """-> (R1CS, full assignment z as ints, rows of the enforced equalities)."""
        cs = CS()
        rows = self.generate_constraints(cs)
        r1cs, z = cs.to_r1cs()
        return r1cs, z, rows


def synthesize(t: ShieldedTransfer):
    return t.synthesize()


def shape_key(t: ShieldedTransfer) -> tuple:
    """(path length per input..., number of outputs): what the matrices, the
    proving key and the witness program depend on."""
    if len(t.nullifiers) != len(t.inputs) or len(t.commitments) != len(t.outputs):
        raise ValueError("one public nullifier per input and one public commitment per output")
    return tuple(min(len(n.merkle_path), len(n.path_bits)) for n in t.inputs) + (len(t.outputs),)


def public_inputs_fr(t: ShieldedTransfer) -> list:
    """The instance values in allocation order, without One (what a verifier feeds)."""
    return [_fr_le(t.merkle_root)] + [_fr_le(x) for x in t.nullifiers] + [_fr_le(x) for x in t.commitments] + \
        [int(t.fee) % R]


def first_unsatisfied(r1cs, z):
    """Lowest row with <a,z><b,z> != <c,z>, or None."""
    def ev(row):
        return sum(c * z[i] for i, c in row) % R
    for k, (a, b, c) in enumerate(zip(r1cs.rows["a"], r1cs.rows["b"], r1cs.rows["c"])):
        if ev(a) * ev(b) % R != ev(c):
            return k
    return None


def z_limbs(z) -> np.ndarray:
    """ints -> (n, 4) canonical u64 limbs."""
    raw = b"".join((int(v) % R).to_bytes(32, "little") for v in z)
    return np.frombuffer(raw, np.uint64).reshape(-1, 4).copy()


# ============================================================ witness program
def pack_pos_word(nterms2: int, mask: int, full: int, partial: int) -> int:
    """Word 3 of a kind-9 op (zkmi.h): third length | mask << 16 | R_p << 19 | R_f/2 << 27."""
    return nterms2 | (mask << 16) | (partial << 19) | ((full // 2) << 27)


def build_program(num_vars, num_instance, input_var, ops, params=None) -> ProgramArrays:
    """ProgramArrays of kind-9 / kind-10 ops given as (kind, out, mask,
    [terms, terms, terms]) with terms = [(z index, coefficient int)].  The
    coefficient table starts with the Poseidon constants (ark[r][i] at 3r + i,
    then mds[i][j]); levels follow wprog.py's rule (1 + the deepest level among
    the variables an op reads; inputs are level 0), permutations first within
    a level."""
    p = params or shielded_params()
    rounds = p["full"] + p["partial"]
    table = [c % R for row in p["ark"] for c in row] + [c % R for row in p["mds"] for c in row]
    assert len(table) == 3 * rounds + 9
    ids: dict = {}

    def cid(c):
        i = ids.get(c)
        if i is None:
            i = ids[c] = len(table)
            table.append(c)
        return i

    level = np.full(num_vars, -1, np.int64)
    level[np.asarray(input_var, np.int64)] = 0
    raw = np.zeros(num_vars, bool)  # trace values the GPU keeps in Montgomery form until the run's end
    sched = []
    for n, (kind, out, mask, lcs) in enumerate(ops):
        reads = [v for lc in lcs for v, _ in lc]
        assert all(level[v] >= 0 for v in reads), "op reads a variable nothing has produced"
        assert not raw[reads].any(), "only the last round's x^5 of a permutation may be read"
        lv = 1 + max([int(level[v]) for v in reads] or [0])
        span = permutation_rows(mask, p) if kind == KIND_POSEIDON_RC else 1
        assert (level[out:out + span] < 0).all(), "variable written twice"
        level[out:out + span] = lv
        if kind == KIND_POSEIDON_RC:
            raw[out:out + span] = True
            raw[[out + span - 9 + k for k in (2, 5, 8)]] = False
        sched.append((lv, kind, n))
    assert (level >= 0).all(), "variables neither inputs nor op outputs"
    sched.sort()
    terms, oparr, lvs = [], np.zeros((len(ops), 4), np.uint32), []
    for i, (lv, kind, n) in enumerate(sched):
        _, out, mask, lcs = ops[n]
        off = len(terms)
        for lc in lcs:
            assert len(lc) < 4096
            terms += [(v, cid(c % R)) for v, c in lc]
        w3 = pack_pos_word(len(lcs[2]), mask, p["full"], p["partial"]) if kind == KIND_POSEIDON_RC else len(lcs[2])
        oparr[i] = (kind | (len(lcs[0]) << 8) | (len(lcs[1]) << 20), out, off, w3)
        lvs.append(lv)
    nlev = max(lvs) if lvs else 0
    level_start = np.searchsorted(np.array(lvs, np.int64), np.arange(1, nlev + 2)).astype(np.uint32)
    coeff = np.frombuffer(b"".join(c.to_bytes(32, "little") for c in table), np.uint64).reshape(-1, 4)
    term = np.array(terms, np.uint32).reshape(-1, 2) if terms else np.zeros((0, 2), np.uint32)
    return ProgramArrays(num_vars, num_instance, input_var, oparr, term, coeff, level_start)


def record(t: ShieldedTransfer):
    """Synthesize with a RecordingCS: (R1CS, z, program, rows).  The program
    (wprog.ProgramArrays, with .template_inputs = this transfer's inputs)
    serves every transfer of t's shape."""
    cs = RecordingCS()
    rows = t.generate_constraints(cs)
    r1cs, z = cs.to_r1cs()
    ni = len(cs.inst)

    def idx(sym):
        return sym[1] if sym[0] == "i" else ni + sym[1]

    input_var = np.array(list(range(ni)) + [ni + w for w in cs.free], np.uint32)
    ops = [(kind, ni + w0, mask, [[(idx(s), k) for s, k in lc.items() if k] for lc in lcs])
           for kind, w0, mask, lcs in cs.ops]
    prog = build_program(len(z), ni, input_var, ops)
    prog.template_inputs = z_limbs([z[int(v)] for v in input_var])
    return r1cs, z, prog, rows


def witness_inputs(t: ShieldedTransfer) -> np.ndarray:
    """The transfer's free inputs in the program's order ((num_inputs, 4)
    canonical u64): One, the public inputs, then the witnesses the circuit
    allocates itself, in allocation order.  No hashing."""
    shape_key(t)
    vals = [1] + public_inputs_fr(t)
    for n in t.inputs:
        vals += [int(n.value), _fr_le(n.randomness), _fr_le(n.owner_pk), int(n.position), _fr_le(n.spending_key)]
        for sib, right in zip(n.merkle_path, n.path_bits):
            vals += [_fr_le(sib), int(bool(right))]
    for o in t.outputs:
        vals += [int(o.value), _fr_le(o.randomness), _fr_le(o.recipient_pk)]
    return z_limbs(vals)


def _int4(row) -> int:
    return sum(int(row[k]) << (64 * k) for k in range(4))


def interpret(program, inputs) -> list:
    """Plain-integer evaluation of a program of kind-9 and kind-10 ops: the
    full assignment z as ints (the reference the GPU run is compared with)."""
    z = [0] * program.num_vars
    for var, row in zip(program.input_var, np.asarray(inputs, np.uint64)):
        z[int(var)] = _int4(row)
    coeff = [_int4(c) for c in program.coeff]
    term = program.term.tolist()

    def ev(off, n):
        return sum(z[v] * coeff[c] for v, c in term[off:off + n]) % R

    for w0, out, off, w3 in program.op.tolist():
        kind, alen, blen, l2 = w0 & 0xFF, (w0 >> 8) & 0xFFF, w0 >> 20, w3 & 0xFFFF
        x = [ev(off, alen), ev(off + alen, blen), ev(off + alen + blen, l2)]
        if kind == KIND_SELECT:
            z[out] = x[1] if x[0] else x[2]
            continue
        if kind != KIND_POSEIDON_RC:
            raise ValueError(f"interpret: op kind {kind}")
        mask, rp, half = (w3 >> 16) & 7, (w3 >> 19) & 0xFF, w3 >> 27
        rounds = 2 * half + rp
        mds = [[coeff[3 * rounds + 3 * i + j] for j in range(3)] for i in range(3)]
        at = out
        for r in range(rounds):
            x = [(x[i] + coeff[3 * r + i]) % R for i in range(3)]
            full = r < half or r >= half + rp
            for i in range(3 if full else 1):
                x2 = x[i] * x[i] % R
                x4 = x2 * x2 % R
                x5 = x4 * x[i] % R
                x[i] = x5
                if r > 0 or (mask >> i) & 1:
                    z[at:at + 3] = [x2, x4, x5]
                    at += 3
            x = [sum(mds[i][j] * x[j] for j in range(3)) % R for i in range(3)]
    return z


# ================================================================ the prover
@dataclass
class ShieldedProof:
    public_inputs: list  # instance values without One (ints)
    a: np.ndarray = field(repr=False)
    b: np.ndarray = field(repr=False)
    c: np.ndarray = field(repr=False)
    proving_time_ms: float = 0.0
    # with check=True: the R1CS check of the witness the proof was made from
    # (as prover.BatchProof); the proof is made either way
    constraints_ok: bool | None = None
    first_unsatisfied: int | None = None

    def compressed(self) -> bytes:
        """128-B arkworks Proof::serialize_compressed."""
        from . import gpu
        return gpu.proof_serialize_compressed(self.a, self.b, self.c)


class ShieldedProver:
    """Key, resident R1CS and witness program of one circuit shape (path
    length per input..., number of outputs), e.g. (32, 32, 2).  Keygen is
    Groth16::circuit_specific_setup over the shape's dummy instance with
    StdRng::seed_from_u64(seed) (keygen.py).  prove_many runs the witness
    program for all transfers at once into a strided z buffer in HBM and
    proves them in one batched call; z never visits the host."""

    def __init__(self, ctx, shape, seed: int = 0, check: bool = False, precompute: bool = True):
        from . import gpu
        from .keygen import circuit_specific_setup
        from .rng import StdRng
        from .wprog import WitnessProgram
        self.ctx, self.shape, self.check = ctx, tuple(shape), check
        self.r1cs, _, self.program, self.rows = record(ShieldedTransfer.dummy(self.shape))
        self.pk, self.verifying_key = circuit_specific_setup(ctx, self.r1cs, StdRng.seed_from_u64(seed))
        if precompute:
            self.pk.precompute()
        self.dev = gpu.R1CSDevice(ctx, self.r1cs)
        self.wp = WitnessProgram(ctx, self.program)
        self.stride = self.program.num_vars * 32
        self._dz = None
        self._vk = None

    def z_buffer(self, nb: int):
        from . import gpu
        if self._dz is None or self._dz.nbytes < nb * self.stride:
            self._dz = gpu.DeviceBuffer(self.ctx, nb * self.stride)
        return self._dz

    def prove_many(self, transfers, seeds) -> list:
        """One ShieldedProof per transfer, in order; proof i's r, s are the first
        two Fr::rand of StdRng::seed_from_u64(seeds[i]) (Groth16Prover's order)."""
        from . import gpu
        from .rng import StdRng
        transfers, seeds = list(transfers), list(seeds)
        nb = len(transfers)
        if len(seeds) != nb:
            raise ValueError("one seed per transfer")
        if not nb:
            return []
        for t in transfers:
            if shape_key(t) != self.shape:
                raise ValueError(f"transfer of shape {shape_key(t)} given to a prover of shape {self.shape}")
        start = time.perf_counter()
        rs, ss = [], []
        for sd in seeds:
            rng = StdRng.seed_from_u64(int(sd))
            rs.append(rng.fr_rand())
            ss.append(rng.fr_rand())
        dz = self.z_buffer(nb)
        self.wp.run_many([witness_inputs(t) for t in transfers], dz, self.stride)
        prev = self.ctx.prove_check()
        if self.check:
            self.ctx.set_prove_check(True)
        try:
            proofs = gpu.groth16_prove_many(self.ctx, self.pk, self.dev, dz, nb, self.stride, rs, ss)
        finally:
            if self.check:
                self.ctx.set_prove_check(prev)
        sts = gpu.groth16_last_check(self.ctx) if self.check else None
        ms = (time.perf_counter() - start) * 1e3 / nb
        out = []
        for k, (t, (a, b, c)) in enumerate(zip(transfers, proofs)):
            extra = {} if sts is None else {"constraints_ok": sts[k].first_row is None,
                                            "first_unsatisfied": sts[k].first_row}
            out.append(ShieldedProof(public_inputs_fr(t), a, b, c, ms, **extra))
        return out

    # ------------------------------------------------------------- verification
    def _resident_vk(self):
        from . import gpu
        if self._vk is None:
            self._vk = gpu.VerifyingKey(self.ctx, self.verifying_key)
        return self._vk

    @staticmethod
    def _split(proofs, public_inputs):
        proofs = list(proofs)
        ins = [p.public_inputs for p in proofs] if public_inputs is None else list(public_inputs)
        return [(p.a, p.b, p.c) for p in proofs], ins

    def verify_many(self, proofs, public_inputs=None) -> list:
        """gpu.groth16_verify_many over the key's resident vk (public_inputs
        default to the proofs' own)."""
        from . import gpu
        pts, ins = self._split(proofs, public_inputs)
        return gpu.groth16_verify_many(self.ctx, self._resident_vk(), pts, ins)[0]

    def verify_each(self, proofs, public_inputs=None) -> list:
        from . import gpu
        pts, ins = self._split(proofs, public_inputs)
        return gpu.groth16_verify_each(self.ctx, self._resident_vk(), pts, ins)[0]

    def verify_many_encoded(self, fmt: int, raws, public_inputs, each: bool = False) -> list:
        """Proofs as wire bytes of format fmt (gpu.PROOF_*), decoded on the GPU."""
        from . import gpu
        fn = gpu.groth16_verify_each_encoded if each else gpu.groth16_verify_many_encoded
        return fn(self.ctx, self._resident_vk(), fmt, raws, public_inputs)[0]

    def close(self):
        for o in (self.wp, self.dev, self.pk, self._vk):
            if o is not None:
                o.close()
        if self._dz is not None:
            self._dz.free()
        self.wp = self.dev = self.pk = self._vk = self._dz = None
