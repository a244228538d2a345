"""The sequencer's account state with its tree on the GPU: what the reference
builds in core/src/sequencer/settlement/prover.rs:580-760
(build_witness_with_proofs) over core/src/sequencer/storage/account_tree.rs,
here over gpu.AccountTreeDevice and gpu.MimcHasher.

DeviceAccountState keeps (pubkey, balance, nonce, position) per account on the
host, where the reference's db keeps them, and the MiMC tree in device memory.
batches() turns lists of transfers and withdrawals into the Prover.toml-shaped
dicts that zbatch.batch_inputs and batch_worker.ZBatchProver take, with no
Python hash: every leaf is one hash_many, every tree write of every batch one
apply, whose per-write siblings and roots are the sender and receiver paths
and the batches' state roots.

Deviations from the reference, on purpose:
  * two different ids on one position raise ValueError (the reference's
    AccountTree overwrites the earlier account's leaf silently);
  * an id that was never inserted raises KeyError (the reference gives it a
    default state and, for a receiver, an extra tree write the circuit does
    not know of);
  * a tree of depth < 32 (reduced circuits) takes the leading `depth` bits of
    the 32-bit position.
zbatch.SparseTree / synthetic_batch / mimc_hash stay what they are: the oracle."""
from __future__ import annotations

from . import gpu, tx_auth
from .r1cs import R


def _ints(arr) -> list:
    return [int.from_bytes(row.tobytes(), "little") for row in arr.reshape(-1, 4)]


class DeviceAccountState:
    def __init__(self, ctx: gpu.Context, depth: int = 32, max_nodes: int = 1 << 20,
                 hasher: gpu.MimcHasher | None = None):
        self.ctx, self.depth = ctx, depth
        self._own_hasher = hasher is None
        self.hasher = hasher if hasher is not None else gpu.MimcHasher(ctx)
        self.tree = gpu.AccountTreeDevice(ctx, self.hasher, depth, max_nodes)
        self.accounts: dict[bytes, list] = {}  # id -> [pubkey, balance, nonce, position]
        self._at: dict[int, bytes] = {}        # position -> id
        # the shielded slots pass through empty: the root synthetic_batch uses
        self.shielded_root = _ints(self.hasher.hash_many([(0, 0)]))[0]

    # ---------------------------------------------------------------- accounts
    def position_of(self, account_id: bytes) -> int:
        """account_tree.rs:322-327: the first four bytes of the id, big-endian
        (their leading `depth` bits in a reduced tree)"""
        return int.from_bytes(bytes(account_id)[:4], "big") >> (32 - self.depth)

    @staticmethod
    def pubkey_of(account_id: bytes) -> int:
        return int.from_bytes(bytes(account_id), "big") % R  # bytes_to_field, account_tree.rs:188-192

    def root(self) -> int:
        return _ints(self.tree.root())[0]

    def insert_many(self, accounts):
        """accounts: (id, balance, nonce) each, new or known (a known one is
        overwritten): one leaf hash_many, then one apply.  -> the root"""
        accounts = [(bytes(a), int(b), int(n)) for a, b, n in accounts]
        claimed = dict(self._at)
        for aid, _, _ in accounts:
            if len(aid) != 32:
                raise ValueError("an account id is 32 bytes")
            pos = self.position_of(aid)
            if claimed.setdefault(pos, aid) != aid:
                raise ValueError(f"accounts {claimed[pos].hex()[:16]}.. and {aid.hex()[:16]}.. share position {pos}")
        if not accounts:
            return self.root()
        leaves = self.hasher.hash_many([(1, self.pubkey_of(a), b, n) for a, b, n in accounts])
        self.tree.apply([self.position_of(a) for a, _, _ in accounts], leaves)
        for aid, bal, nonce in accounts:
            pos = self.position_of(aid)
            self.accounts[aid] = [self.pubkey_of(aid), bal, nonce, pos]
            self._at[pos] = aid
        return self.root()

    def insert(self, account_id: bytes, balance: int, nonce: int = 0):
        """the deposit path (AccountTree::insert)"""
        return self.insert_many([(account_id, balance, nonce)])

    # ----------------------------------------------------------------- batches
    @staticmethod
    def _authorise(batches, verifier):
        """the signed entries of all batches through one verify_signed; a
        refused one raises ValueError.  -> the batches with tuples throughout"""
        signed = [(b["batch_id"], kind, i, e) for b in batches for kind in ("transfers", "withdrawals")
                  for i, e in enumerate(b.get(kind, [])) if isinstance(e, (tx_auth.SignedTransfer, tx_auth.SignedWithdrawal))]
        if not signed:
            return batches
        if verifier is None:
            raise ValueError("signed transfers and withdrawals need a verifier")
        for bid, kind, i, e in signed:
            if isinstance(e, tx_auth.SignedTransfer) != (kind == "transfers"):
                raise ValueError(f"batch {bid}: {kind}[{i}] is a {type(e).__name__}")
        reasons, _ = tx_auth.verify_signed(verifier, [e for *_, e in signed])
        for (bid, kind, i, _), reason in zip(signed, reasons):
            if reason != tx_auth.OK:
                raise ValueError(f"batch {bid}: {kind}[{i}] refused: {reason}")
        as_tuple = lambda e: (tx_auth.transfer_tuple(e) if isinstance(e, tx_auth.SignedTransfer) else
                              tx_auth.withdrawal_tuple(e) if isinstance(e, tx_auth.SignedWithdrawal) else e)
        return [{**b, "transfers": [as_tuple(e) for e in b.get("transfers", [])],
                 "withdrawals": [as_tuple(e) for e in b.get("withdrawals", [])]} for b in batches]

    def batches(self, batches, max_transfers: int = 8, max_withdrawals: int = 4, verifier=None):
        """batches: [{"batch_id": int, "transfers": [(sender id, receiver id,
        amount, signature)], "withdrawals": [(sender id, l1_recipient, amount,
        signature)]}], applied in order, the transfers of a batch before its
        withdrawals (main.nr's order).  -> one Prover.toml-shaped dict per
        batch.  The state (host accounts and device tree) advances past all of
        them.  A batch with more transfers than max_transfers or more
        withdrawals than max_withdrawals (the circuit's slot counts) raises
        ValueError, an unknown id KeyError; both before anything changes.
        Amounts, signatures and ids may be any integer type.

        verifier (a gpu.Ed25519Verifier, or anything with its verify_many):
        an entry may then be a tx_auth.SignedTransfer or SignedWithdrawal in
        place of a tuple.  The signatures of all batches are checked in one
        pass (tx_auth.verify_signed: the readable message first, the legacy
        one for the failures) before anything changes, and a refused one
        raises ValueError naming the batch, the index and the reason.  With a
        gpu.Ed25519Verifier that pass takes tx_auth's device path: the entries
        go to the device as fixed-width records, and the messages are built,
        verified, retried and `from` compared there (zkmi_tx_auth_many); a
        verifier with verify_many alone takes the host path.  The
        circuit's `signature` input then carries the first 31 bytes of the
        signature as a big-endian integer (tx_auth.signature_field): a
        pass-through value the circuit does not constrain; the check that
        counts is the one made here.  Nonces and balances are not judged here,
        with or without a verifier.  Without a verifier nothing differs from
        before, and a signed entry raises ValueError."""
        depth = self.depth
        batches = self._authorise(list(batches), verifier)
        norm = []
        for b in batches:
            ts = [(bytes(s), bytes(r), int(amount), int(sig)) for s, r, amount, sig in b.get("transfers", [])]
            ws = [(bytes(s), int(l1), int(amount), int(sig)) for s, l1, amount, sig in b.get("withdrawals", [])]
            if len(ts) > max_transfers or len(ws) > max_withdrawals:
                raise ValueError(f"batch {b['batch_id']}: {len(ts)} transfers and {len(ws)} withdrawals for "
                                 f"{max_transfers} and {max_withdrawals} slots")
            for aid in [x for t in ts for x in t[:2]] + [w[0] for w in ws]:
                if aid not in self.accounts:
                    raise KeyError(f"account {aid.hex()[:16]}.. was never inserted")
            norm.append({"batch_id": int(b["batch_id"]), "transfers": ts, "withdrawals": ws})
        batches = norm
        st = {}  # walked copies of the touched accounts

        def acct(aid):
            aid = bytes(aid)
            if aid not in st:
                st[aid] = list(self.accounts[aid])
            return st[aid]

        # 1. balances and nonces, as integers; every write in order
        plan, w_pos, w_leaf = [], [], []
        for b in batches:
            first = len(w_pos)
            ts, ws = [], []
            for s, r, amount, sig in b["transfers"]:
                a = acct(s)
                spk, sbal, snonce, spos = a
                a[1:3] = [max(0, sbal - amount), snonce + 1]
                w_pos.append(spos)
                w_leaf.append((1, spk, a[1], a[2]))
                c = acct(r)
                rpk, rbal, rnonce, rpos = c
                c[1] = rbal + amount
                w_pos.append(rpos)
                w_leaf.append((1, rpk, c[1], rnonce))
                ts.append({"sender_pubkey": spk, "sender_balance": sbal, "sender_nonce": snonce,
                           "receiver_pubkey": rpk, "receiver_balance": rbal, "receiver_nonce": rnonce,
                           "amount": amount, "signature": sig, "is_valid": True,
                           "_w": (len(w_pos) - 2, len(w_pos) - 1)})
            for s, l1, amount, sig in b["withdrawals"]:
                a = acct(s)
                spk, sbal, snonce, spos = a
                a[1:3] = [max(0, sbal - amount), snonce + 1]
                w_pos.append(spos)
                w_leaf.append((1, spk, a[1], a[2]))
                ws.append({"sender_pubkey": spk, "sender_balance": sbal, "sender_nonce": snonce,
                           "l1_recipient": l1, "amount": amount, "signature": sig, "is_valid": True,
                           "_w": (len(w_pos) - 1,)})
            plan.append((int(b["batch_id"]), ts, ws, first, len(w_pos)))

        # 2. all new leaves: one hash_many; all writes of all batches: ONE apply
        root0 = self.root()
        if w_pos:
            sib, _, roots = self.tree.apply(w_pos, self.hasher.hash_many(w_leaf))
            roots = _ints(roots)
            sib = [_ints(s) for s in sib]
        bits = [[(p >> lv) & 1 for lv in range(depth)] for p in w_pos]

        # 3. transaction and withdrawal hashes: one hash_many each
        tx = [(t["sender_pubkey"], t["receiver_pubkey"], t["amount"], t["sender_nonce"]) for _, ts, _, _, _ in plan for t in ts]
        wd = [(w["l1_recipient"], w["amount"], w["sender_pubkey"]) for _, _, ws, _, _ in plan for w in ws]
        tx_h = _ints(self.hasher.hash_many(tx)) if tx else []
        wd_h = _ints(self.hasher.hash_many(wd)) if wd else []

        # 4. the accumulators: every batch's chain advances one link a round
        nb = len(plan)
        heads = _ints(self.hasher.hash_many([(4, bid) for bid, *_ in plan] + [(5, bid) for bid, *_ in plan])) if nb else []
        b_acc, w_acc = heads[:nb], heads[nb:]
        links, ti, wi = [], 0, 0  # per batch: [(hash, amount, is_withdrawal)]
        for _, ts, ws, _, _ in plan:
            links.append([(tx_h[ti + i], t["amount"], False) for i, t in enumerate(ts)] +
                         [(wd_h[wi + i], w["amount"], True) for i, w in enumerate(ws)])
            ti, wi = ti + len(ts), wi + len(ws)
        for step in range(max((len(x) for x in links), default=0)):
            live = [i for i in range(nb) if step < len(links[i])]
            got = _ints(self.hasher.hash_many([(b_acc[i], links[i][step][0], links[i][step][1]) for i in live]))
            for i, v in zip(live, got):
                b_acc[i] = v
            wlive = [i for i in live if links[i][step][2]]
            if wlive:
                got = _ints(self.hasher.hash_many([(w_acc[i], links[i][step][0]) for i in wlive]))
                for i, v in zip(wlive, got):
                    w_acc[i] = v
        if nb:
            b_fin = _ints(self.hasher.hash_many([(b_acc[i], len(plan[i][1]), len(plan[i][2]), 0) for i in range(nb)]))
            w_fin = _ints(self.hasher.hash_many([(w_acc[i], len(plan[i][2])) for i in range(nb)]))

        # 5. the dicts
        out = []
        for i, (bid, ts, ws, first, end) in enumerate(plan):
            for t in ts:
                ks, kr = t.pop("_w")
                t["sender_path"], t["sender_path_indices"] = sib[ks], bits[ks]
                t["receiver_path"], t["receiver_path_indices"] = sib[kr], bits[kr]
            for w in ws:
                (ks,) = w.pop("_w")
                w["sender_path"], w["sender_path_indices"] = sib[ks], bits[ks]
            pre = roots[first - 1] if first else root0
            post = roots[end - 1] if end else root0
            out.append({"pre_state_root": pre, "post_state_root": post, "pre_shielded_root": self.shielded_root,
                        "post_shielded_root": self.shielded_root, "withdrawal_root": w_fin[i], "batch_hash": b_fin[i],
                        "batch_id": bid, "num_transfers": len(ts), "num_withdrawals": len(ws), "num_shielded": 0,
                        "transfers": ts, "withdrawals": ws, "shielded": []})
        for aid, a in st.items():
            self.accounts[aid] = a
        return out

    def close(self):
        self.tree.close()
        if self._own_hasher:
            self.hasher.close()
