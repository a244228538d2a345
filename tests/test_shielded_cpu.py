"""ShieldedTransferCircuit (zelana_amd/shielded.py) on the host: parameters,
honest and tampered transfers against the R1CS, the closed-form row count, and
the recorded witness program against the synthesis assignment.

The R1CS is parity-unpinned (see shielded.py): what is checked is what the
circuit must do whatever the gadget internals are.
"""
import copy

import numpy as np
import pytest

from zelana_amd import shielded as S
from zelana_amd.l2block import _PARAMS, GrainLFSR, poseidon_params
from zelana_amd.r1cs import R


def _b(x):
    return bytes([x] * 32)


def _notes(depth, n_in, n_out, salt=0):
    """An honest transfer: n_in notes of one tree (so they share the root), n_out outputs, fee 3."""
    tree = S.NoteTree(depth)
    tree.insert(0, 12345)  # a foreign leaf, so siblings are not all empty subtrees
    vals = [100 + salt, 50 + 2 * salt][:n_in]
    pos = [1, (1 << depth) - 2][:n_in]
    ins = tree.spend_notes([(v, _b(10 + i + salt), _b(20 + i + salt), p) for i, (v, p) in enumerate(zip(vals, pos))])
    total = sum(vals) - 3
    outs = [S.OutputNote(total - 7 * (n_out - 1), _b(30 + salt), _b(40))] + \
        [S.OutputNote(7, _b(31 + k + salt), _b(41 + k)) for k in range(n_out - 1)]
    return S.ShieldedTransfer.honest(ins, outs)


@pytest.fixture(scope="module")
def t22():
    """(2,2) depth 2: the transfer, its recording synthesis, shared by the tests below (read only)."""
    t = _notes(2, 2, 2)
    return (t,) + S.record(t)


def test_package_exports_the_prover():
    import zelana_amd
    assert zelana_amd.ShieldedProver is S.ShieldedProver and "ShieldedProver" in zelana_amd.__all__
    with pytest.raises(AttributeError):
        zelana_amd.no_such_name


# ------------------------------------------------------------------ parameters
def test_shielded_parameters_differ_from_l2():
    p, l2 = S.shielded_params(), poseidon_params()
    assert len(p["ark"]) == 65 and all(len(r) == 3 for r in p["ark"])
    assert len(p["mds"]) == 3 and all(len(r) == 3 for r in p["mds"])
    assert (p["full"], p["partial"], p["rate"], p["capacity"], p["alpha"]) == (8, 57, 2, 1, 5)
    assert len(l2["ark"]) == 64 and p["ark"][0] != l2["ark"][0] and p["mds"] != l2["mds"]
    assert all(0 <= c < R for row in p["ark"] + p["mds"] for c in row)


def test_l2_parameters_unchanged():
    """poseidon_params() is what it was before the prime_bits keyword: the
    254-bit Grain stream, rejection-sampled, then the Cauchy matrix."""
    got = poseidon_params()
    lfsr = GrainLFSR(254, 3, 8, 56)
    ark = []
    for _ in range(64):
        row = []
        while len(row) < 3:
            v = 0
            for b in lfsr.get_bits(254):
                v = (v << 1) | int(b)
            if v < R:
                row.append(v)
        ark.append(row)
    xs, ys = lfsr.field_elements_mod_p(3), lfsr.field_elements_mod_p(3)
    mds = [[pow((xs[i] + ys[j]) % R, R - 2, R) for j in range(3)] for i in range(3)]
    assert got["ark"] == ark and got["mds"] == mds
    assert got == dict(ark=ark, mds=mds, rate=2, capacity=1, full=8, partial=56, alpha=5)
    assert poseidon_params(prime_bits=254) is got and (2, 8, 56, 5, 0, 254) in _PARAMS


# ------------------------------------------------------------ honest transfers
@pytest.mark.parametrize("depth,n_in,n_out,rows", [(2, 1, 1, 2174), (2, 2, 1, None), (2, 1, 2, None),
                                                   (2, 2, 2, 4347), (32, 2, 2, 18927)])
def test_honest_transfer_satisfies(depth, n_in, n_out, rows):
    t = _notes(depth, n_in, n_out)
    assert all(n.merkle_path and len(n.merkle_path) == depth for n in t.inputs)
    assert len({S.merkle_root(S.note_commitment(n.value, n.randomness, n.owner_pk), n.merkle_path, n.path_bits)
                for n in t.inputs}) == 1, "inputs share one root"
    cs, z, eq = S.synthesize(t)
    assert S.first_unsatisfied(cs, z) is None
    assert cs.num_instance == 3 + n_in + n_out
    assert z[1:cs.num_instance] == S.public_inputs_fr(t)
    want = S.expected_rows(S.shape_key(t))
    assert cs.num_constraints == want and (rows is None or want == rows)
    if depth == 32:
        assert 1 << 14 < cs.num_constraints + cs.num_instance <= 1 << 15
        assert S.expected_rows((32, 1)) == 9464
    assert len(eq["root"]) == len(eq["nullifier"]) == len(eq["pk"]) == n_in and len(eq["commitment"]) == n_out


# --------------------------------------------------------------- tamper classes
def _tampered(t, what):
    """(tampered copy, name of the equality it breaks, index of that equality)"""
    t = copy.deepcopy(t)
    if what == "nullifier":
        t.nullifiers[1] = S._b32(S._fr_le(t.nullifiers[1]) + 1)
        return t, "nullifier", 1
    if what == "root":
        t.merkle_root = S._b32(S._fr_le(t.merkle_root) + 1)
        return t, "root", 0
    if what == "sibling":
        t.inputs[1].merkle_path[0] = S._b32(S._fr_le(t.inputs[1].merkle_path[0]) + 1)
        return t, "root", 1
    if what == "path_bit":
        t.inputs[0].path_bits[1] = not t.inputs[0].path_bits[1]
        return t, "root", 0
    if what == "spending_key":  # another key, with the nullifier it gives: only the owner check fails
        n = t.inputs[1]
        n.spending_key = _b(99)
        t.nullifiers[1] = S._b32(S.nullifier(n.spending_key, S.note_commitment(n.value, n.randomness, n.owner_pk),
                                             n.position))
        return t, "pk", 1
    if what == "commitment":
        t.commitments[1] = S._b32(S._fr_le(t.commitments[1]) + 1)
        return t, "commitment", 1
    assert what == "fee"
    t.fee += 1
    return t, "balance", None


TAMPERS = ["nullifier", "root", "sibling", "path_bit", "spending_key", "commitment", "fee"]


@pytest.mark.parametrize("what", TAMPERS)
def test_tampered_transfer_fails_at_its_equality(t22, what):
    bad, name, k = _tampered(t22[0], what)
    cs, z, eq = S.synthesize(bad)
    row = eq[name] if k is None else eq[name][k]
    assert S.first_unsatisfied(cs, z) == row
    assert eq == t22[4], "the equalities sit at the same rows for every transfer of the shape"


# --------------------------------------------------------------------- program
def test_program_reproduces_synthesis(t22):
    t, cs, z, prog, _ = t22
    assert set(prog.kinds.tolist()) == {S.KIND_POSEIDON_RC, S.KIND_SELECT}
    masks = set(((prog.op[:, 3] >> 16) & 7)[prog.kinds == S.KIND_POSEIDON_RC].tolist())
    assert masks == {4, 6, 7}
    assert np.array_equal(prog.template_inputs, S.witness_inputs(t))
    assert prog.num_vars == len(z) and prog.num_instance == cs.num_instance
    assert S.interpret(prog, prog.template_inputs) == z
    others = [_notes(2, 2, 2, salt=5), _tampered(t, "sibling")[0], _tampered(_notes(2, 2, 2, salt=9), "fee")[0]]
    for o in others:
        assert S.shape_key(o) == S.shape_key(t)
        assert S.interpret(prog, S.witness_inputs(o)) == S.synthesize(o)[1]


def test_program_levels_and_layout(t22):
    _, _, z, prog, _ = t22
    ls = prog.level_start
    assert ls[0] == 0 and ls[-1] == prog.op.shape[0] and (np.diff(ls.astype(np.int64)) > 0).all()
    ready = np.zeros(prog.num_vars, bool)
    ready[prog.input_var] = True
    rounds = 65
    assert prog.coeff.shape[0] >= 3 * rounds + 9
    for l in range(prog.num_levels):
        written = []
        kinds = prog.kinds[ls[l]:ls[l + 1]].tolist()
        assert kinds == sorted(kinds), "permutations first within a level"
        for w0, out, off, w3 in prog.op[ls[l]:ls[l + 1]].tolist():
            n = ((w0 >> 8) & 0xFFF) + (w0 >> 20) + (w3 & 0xFFFF)
            assert ready[prog.term[off:off + n, 0]].all(), "an op reads only inputs and earlier levels"
            if w0 & 0xFF == S.KIND_POSEIDON_RC:
                assert (w3 >> 27, (w3 >> 19) & 0xFF) == (4, 57)
                span = S.permutation_rows((w3 >> 16) & 7)
                written += [out + span - 9 + k for k in (2, 5, 8)]  # only the last round's x^5 may be read
            else:
                assert w3 >> 16 == 0
                written.append(out)
        ready[written] = True


def test_shape_keys_separate_shapes():
    keys = {S.shape_key(S.ShieldedTransfer.dummy(sh)): sh for sh in [(2, 1), (2, 2, 1), (2, 2), (2, 2, 2), (3, 2, 2),
                                                                      (2, 3, 2), (32, 32, 2)]}
    assert len(keys) == 7 and all(k == v for k, v in keys.items())
    t = S.ShieldedTransfer.dummy((3, 1))
    t.inputs[0].path_bits = t.inputs[0].path_bits[:2]  # zip(path, bits) truncates to the shorter
    assert S.shape_key(t) == (2, 1) and S.synthesize(t)[0].num_constraints == S.expected_rows((2, 1))
    t.nullifiers = []
    with pytest.raises(ValueError):
        S.shape_key(t)
    with pytest.raises(ValueError):
        S.synthesize(t)


def test_dummy_matrices_are_the_shapes(t22):
    """keygen runs over the dummy instance: same matrices as any transfer of the shape"""
    t, cs, _, prog, _ = t22
    d_cs, _, d_prog, _ = S.record(S.ShieldedTransfer.dummy(S.shape_key(t)))
    assert d_cs.rows == cs.rows
    for name in ("op", "term", "coeff", "level_start", "input_var"):
        assert np.array_equal(getattr(d_prog, name), getattr(prog, name)), name
