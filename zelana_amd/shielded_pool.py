"""ShieldedPool: the sequencer's side of the shielded path, one call for a pile.

The reference accepts a shielded transaction only if its root is current or
recent, none of its nullifiers has been spent (in persistent state or earlier
in the same batch) and its proof verifies; only then are its commitments
appended and its nullifiers marked spent (core/src/sequencer/execution/
tx_router.rs:219-346, storage/shielded_state.rs:89-175).  ShieldedPool holds
that state on the GPU: the note commitment tree (shielded.DeviceNoteTree), the
spent-nullifier set (gpu.NullifierSetDevice) and the resident
verifying key; settle() turns wire-format proofs plus public inputs into
per-transfer verdicts and updated pool state.  Given the transfers' encrypted
output notes as well, settle() stores those of the accepted transfers beside
their commitments (gpu.NoteStoreDevice) and scan() answers a
wallet's "which notes are mine" in one call.

Two rules of settle() differ from, or go beyond, a one-by-one replay of the
reference; both are deliberate:

  * Canonical bytes.  The verifier reads public inputs mod r, the nullifier
    set compares bytes.  nf and nf + r verify under the same proof and would
    count as two different nullifiers (r is about 2^253.8: up to five aliases
    of a value fit 32 bytes), so a transfer whose root, nullifier, commitment
    or fee bytes encode a value >= r is refused as NONCANONICAL and left out
    of the verify call, which refuses a whole pile over one such input.
  * Roots are judged against the history as it stands when the call begins.
    In a strict replay every accepted transfer pushes its commitments' roots,
    so a root from before the call can leave the history of 100 after 50
    accepted two-output transfers.  The reference never meets the case: it
    seals a batch at max_shielded = 10 (execution/batch.rs:57-68).
"""
from __future__ import annotations

from dataclasses import dataclass, field

from .r1cs import R

ACCEPTED, NONCANONICAL, BAD_ROOT, BAD_ENCODING, BAD_PROOF = "ACCEPTED", "NONCANONICAL", "BAD_ROOT", "BAD_ENCODING", \
    "BAD_PROOF"
SPENT_STORED, SPENT_IN_CALL, DUP_IN_TX = "SPENT_STORED", "SPENT_IN_CALL", "DUP_IN_TX"
NONE, MIMC, POSEIDON = 0, 1, 2  # commitment schemes of scan (gpu.COMMIT_*)


@dataclass
class Settlement:
    """The verdict on one transfer of a pile.  status: ACCEPTED, or why not:
    NONCANONICAL, BAD_ROOT, BAD_ENCODING (a malformed proof encoding),
    BAD_PROOF (the proof, an invalid point included, does not verify),
    SPENT_STORED (detail = which nullifier was spent before the call),
    SPENT_IN_CALL (detail = the earlier transfer of the pile that spent one),
    DUP_IN_TX (detail = which nullifier repeats an earlier one of the
    transfer).  An accepted transfer carries the positions of its output
    commitments and the root after the last of them."""
    status: str
    detail: int | None = None
    positions: list = field(default_factory=list)
    root: int | None = None

    @property
    def accepted(self) -> bool:
        return self.status == ACCEPTED


def _b32(v) -> bytes:
    if isinstance(v, int):
        return v.to_bytes(32, "little")
    b = bytes(v)
    if len(b) != 32:
        raise ValueError("public inputs are 32-byte values")
    return b


class ShieldedPool:
    """Note tree, nullifier set and verifying key of one shielded pool on one
    context.  prover_or_vk: a shielded.ShieldedProver (its shape gives the
    numbers of nullifiers and commitments, its resident key is used and stays
    its own), or a gpu.VerifyingKey / arkworks-compressed key bytes with n_in
    and n_out given (default: half of the key's inputs each, less root and
    fee)."""

    def __init__(self, ctx, prover_or_vk, depth: int = 32, capacity: int = 1 << 20,
                 nullifier_capacity: int = 1 << 20, empty_leaf=None, n_in: int | None = None,
                 n_out: int | None = None, max_ct: int = 570):
        from . import gpu
        from .shielded import DeviceNoteTree
        self.ctx = ctx
        self._own_vk = False
        if hasattr(prover_or_vk, "_resident_vk"):
            self.vk = prover_or_vk._resident_vk()
            shape = prover_or_vk.shape
            n_in, n_out = (len(shape) - 1 if n_in is None else n_in), (shape[-1] if n_out is None else n_out)
        elif isinstance(prover_or_vk, gpu.VerifyingKey):
            self.vk = prover_or_vk
        else:
            self.vk, self._own_vk = gpu.VerifyingKey(ctx, prover_or_vk), True
        if n_in is None or n_out is None:
            rest = self.vk.n_inputs - 2
            n_in = rest // 2 if n_in is None else n_in
            n_out = rest - n_in if n_out is None else n_out
        if n_in < 1 or n_in > 4 or n_out < 0 or 2 + n_in + n_out != self.vk.n_inputs:
            raise ValueError(f"a key of {self.vk.n_inputs} public inputs does not fit {n_in} nullifiers (1..4) and "
                             f"{n_out} commitments beside root and fee")
        self.n_in, self.n_out = n_in, n_out
        self.tree = DeviceNoteTree(ctx, depth=depth, capacity=capacity, empty_leaf=empty_leaf)
        self.nullifiers = gpu.NullifierSetDevice(ctx, nullifier_capacity)
        # the encrypted-note store: one note per leaf of the tree at most; made by the first call that needs it
        self.max_ct, self._notes, self._mimc = max_ct, None, None

    @property
    def notes(self):
        """the pool's gpu.NoteStoreDevice (capacity = the tree's, ciphertexts up to max_ct bytes)"""
        if self._notes is None:
            from . import gpu
            self._mimc = gpu.MimcHasher(self.ctx)
            self._notes = gpu.NoteStoreDevice(self.ctx, self.tree.dev.capacity, self.max_ct, mimc=self._mimc,
                                              poseidon=self.tree.hasher)
        return self._notes

    # ---------------------------------------------------------------- settle
    def settle(self, fmt: int, raw_proofs, public_inputs, each: bool = False, encrypted_notes=None) -> list:
        """One pile, in order -> [Settlement per transfer].  raw_proofs: the
        proofs as wire bytes of format fmt (gpu.PROOF_*), back to back or as a
        list; public_inputs: per transfer root, nullifiers, commitments, fee
        (shielded.public_inputs_fr's order) as 32-byte little-endian strings
        or ints below 2^256.  each=True takes exact per-proof verdicts
        (verify_each) where the default is the batched check (verify_many).

        In order: non-canonical bytes are refused; roots are checked against
        the history as it stands when the call begins (see the module text);
        the survivors' proofs are verified in one call; the nullifiers of all
        transfers go through one ordered spend in which only the transfers
        that passed so far take part (first one wins; a refused transfer
        spends nothing); the commitments of the accepted transfers are
        appended in order by one append, and every new root enters the
        history.  Raises ZkmiError, with nothing changed, when the pile could
        overflow the tree or the accepted nullifiers do not fit the set.

        encrypted_notes (optional): per transfer, one (ephemeral_pk, nonce,
        ciphertext) per output commitment.  The notes of the ACCEPTED
        transfers are stored at the positions their commitments received, in
        the same call; a refused transfer stores nothing.  Their shapes are
        checked before anything changes (ValueError).  Without the keyword no
        note is stored and nothing else differs."""
        from . import gpu
        from ._lib import ZkmiError
        buf, nb = gpu._encoded(fmt, raw_proofs)
        plen = gpu.proof_encoded_len(fmt)
        public_inputs = list(public_inputs)
        width = 2 + self.n_in + self.n_out
        if len(public_inputs) != nb or any(len(x) != width for x in public_inputs):
            raise ValueError(f"{nb} proofs need {nb} x {width} public inputs")
        if encrypted_notes is not None:
            encrypted_notes = [[(bytes(e), bytes(nc), bytes(ct)) for e, nc, ct in x] for x in encrypted_notes]
            if len(encrypted_notes) != nb or any(len(x) != self.n_out for x in encrypted_notes):
                raise ValueError(f"{nb} transfers need {nb} x {self.n_out} encrypted notes")
            if any(len(e) != 32 or len(nc) != 12 or len(ct) > self.max_ct for x in encrypted_notes for e, nc, ct in x):
                raise ValueError(f"an encrypted note is a 32-byte key, a 12-byte nonce and at most {self.max_ct} "
                                 "bytes of ciphertext")
        rows = [[_b32(v) for v in x] for x in public_inputs]  # 1. split: the 32-byte forms
        vals = [[int.from_bytes(b, "little") for b in row] for row in rows]
        status: list = [None] * nb
        for t in range(nb):
            if any(v >= R for v in vals[t]):  # 2. canonical bytes
                status[t] = NONCANONICAL
            elif not self.tree.is_valid_root(vals[t][0]):  # 3. the history as the call finds it
                status[t] = BAD_ROOT
        live = [t for t in range(nb) if status[t] is None]
        if live:  # 4. proofs
            raws = b"".join(buf[t * plen:(t + 1) * plen].tobytes() for t in live)
            fn = gpu.groth16_verify_each_encoded if each else gpu.groth16_verify_many_encoded
            valid, malformed, _ = fn(self.ctx, self.vk, fmt, raws, [vals[t] for t in live])
            for t, ok, mal in zip(live, valid, malformed):
                if mal:
                    status[t] = BAD_ENCODING
                elif not ok:
                    status[t] = BAD_PROOF
        eligible = [s is None for s in status]
        if self.tree.next_position + sum(eligible) * self.n_out > self.tree.dev.capacity:
            raise ZkmiError(f"settle: {sum(eligible)} transfers of {self.n_out} commitments could pass the tree's "
                            f"capacity {self.tree.dev.capacity} from {self.tree.next_position}")
        if encrypted_notes is not None and self.notes.count + sum(eligible) * self.n_out > self.notes.capacity:
            raise ZkmiError(f"settle: {sum(eligible)} transfers of {self.n_out} notes could pass the note store's "
                            f"capacity {self.notes.capacity} from {self.notes.count}")
        keys = [nf for row in rows for nf in row[1:1 + self.n_in]]  # 5. nullifiers
        verdicts, details, _ = self.nullifiers.spend(keys, self.n_in, eligible) if nb else ([], [], 0)
        names = {gpu.NF_SPENT_STORED: SPENT_STORED, gpu.NF_SPENT_IN_CALL: SPENT_IN_CALL, gpu.NF_DUP_IN_TX: DUP_IN_TX}
        out: list = [None] * nb
        accepted = []
        for t in range(nb):
            if status[t] is not None:
                out[t] = Settlement(status[t])
            elif verdicts[t] == gpu.NF_ACCEPTED:
                accepted.append(t)
            else:
                out[t] = Settlement(names[verdicts[t]], details[t])
        if accepted:  # 6. append
            leaves = [v for t in accepted for v in vals[t][1 + self.n_in:1 + self.n_in + self.n_out]]
            first, roots = self.tree.append(leaves) if leaves else (self.tree.next_position, [])
            for j, t in enumerate(accepted):
                pos = list(range(first + j * self.n_out, first + (j + 1) * self.n_out))
                out[t] = Settlement(ACCEPTED, None, pos, roots[(j + 1) * self.n_out - 1] if self.n_out else None)
            if encrypted_notes is not None and leaves:  # 7. the notes, beside their commitments
                self.notes.append([(out[t].positions[k], rows[t][1 + self.n_in + k]) + encrypted_notes[t][k]
                                   for t in accepted for k in range(self.n_out)])
        return out

    # ------------------------------------------------------------------ scan
    def scan(self, decryption_key, owner_pk, from_position: int = 0, limit: int = 1000, scheme: int = POSEIDON):
        """The stored notes at positions >= from_position that decryption_key
        opens and whose commitment, recomputed under owner_pk by `scheme`
        (POSEIDON: what this pool's tree holds; MIMC: the reference's
        scan_notes handler; NONE: no check), equals the stored one ->
        ([gpu.ScannedNote] in ascending position order, at most limit;
        scanned_to; stats).  A memo comes back as str, or None when it is
        empty or not UTF-8.  When more than limit notes match, scanned_to is
        the position of the last one returned: continue from scanned_to + 1."""
        if self._notes is None:
            return [], from_position, [0, 0, 0, 0]
        hits, scanned_to, stats = self.notes.scan([_b32(decryption_key)], [_b32(owner_pk)], scheme, from_position,
                                                  limit)[0]
        for h in hits:
            try:
                h.memo = h.memo.decode("utf-8") if h.memo else None
            except UnicodeDecodeError:
                h.memo = None
        return hits, scanned_to, stats

    # ------------------------------------------------------------ delegates
    def nullifier_exists(self, nf) -> bool:
        return self.nullifiers.contains([_b32(nf)])[0]

    def spent_log(self, first: int = 0, n: int | None = None) -> list:
        """the spent nullifiers [first, first + n) in the order they were spent (what a restart loads)"""
        return self.nullifiers.log(first, self.nullifiers.count - first if n is None else n)

    def root(self) -> int:
        return self.tree.root()

    def is_valid_root(self, root) -> bool:
        return self.tree.is_valid_root(root)

    def paths(self, positions) -> list:
        return self.tree.paths(positions)

    def close(self):
        if self._notes is not None:
            self._notes.close()
            self._mimc.close()
        self.nullifiers.close()
        self.tree.close()
        if self._own_vk:
            self.vk.close()
