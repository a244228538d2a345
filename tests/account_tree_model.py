"""Inputs and oracles shared by the account-tree tests (test_mimc_hash_cpu.py,
test_gpu_account_tree.py): the write sequences, their one-leaf-at-a-time
results over zbatch.SparseTree (computed once per process and left unchanged),
brute-force checks of the properties the sequences claim, and a host
restatement of the reference sequencer's build_witness_with_proofs
(core/src/sequencer/settlement/prover.rs:580-760) over SparseTree, the oracle
of account_state.DeviceAccountState.batches."""
import functools
import random

import numpy as np

from zelana_amd import zbatch as Z
from zelana_amd.r1cs import R

SPECIALS = [0, R - 1, R, 2**256 - 1]
EDGE32 = [0, 1, 2**32 - 1, 2**32 - 2, 2**31, 2**31 + 1]


def fe_hex(v: int) -> str:
    return int(v).to_bytes(32, "little").hex()


def hex_fe(s: str) -> int:
    return int.from_bytes(bytes.fromhex(s), "little")


def words(vals) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy()


def ints(arr) -> list:
    a = np.ascontiguousarray(arr, np.uint64).reshape(-1, 4)
    return [int.from_bytes(row.tobytes(), "little") for row in a]


@functools.lru_cache(maxsize=None)
def H(*xs: int) -> int:
    return Z.mimc_hash(*[x % R for x in xs])


def hash_inputs(arity: int, n: int, seed: int) -> list:
    """n tuples: the specials first (each in every slot of some tuple), then
    values below r and arbitrary 256-bit values, alternating"""
    rnd = random.Random(1000 * arity + seed)
    out = []
    for i in range(n):
        t = [rnd.randrange(R) if (i + k) & 1 else rnd.getrandbits(256) for k in range(arity)]
        if i < len(SPECIALS) * arity:
            t[i % arity] = SPECIALS[i // arity]
        out.append(tuple(t))
    return out


# ------------------------------------------------------------ write sequences
def _leaf(rnd, i):
    return rnd.randrange(1, R) if i & 1 else rnd.getrandbits(256) | (1 << 255)  # odd: < r; even: >= r


def _prefix(rnd, a, b, c, d, e):
    """the structured writes every sequence carries: a written twice in a row,
    the level-0 pair (b, b^1) left then right, the pair (c, c^1) right then
    left, d written to 0, e written with a value >= r.  a..e: positions."""
    return [(a, _leaf(rnd, 1)), (a, _leaf(rnd, 3)), (b & ~1, _leaf(rnd, 1)), (b | 1, _leaf(rnd, 0)),
            (c | 1, _leaf(rnd, 1)), (c & ~1, _leaf(rnd, 1)), (d, 0), (e, R + 5)]


def _seq_depth3():
    rnd = random.Random(3)
    w = _prefix(rnd, 0, 2, 4, 1, 6) + [(7, _leaf(rnd, 1))]
    w += [(rnd.randrange(8), _leaf(rnd, i)) for i in range(20 - len(w))]
    return w


def _seq_depth32(sizes, seed):
    """consecutive calls of the given sizes over the edge positions, their
    neighbours and random positions; every call after the first starts with a
    write whose level-0 sibling was stored by the call before it"""
    rnd = random.Random(seed)
    pool = EDGE32 + [rnd.getrandbits(32) for _ in range(12)]
    pool += [p ^ 1 for p in pool[6:10]] + [p ^ (1 << 31) for p in pool[10:12]] + [p ^ (1 << 16) for p in pool[12:14]]
    calls = []
    for ci, n in enumerate(sizes):
        if ci == 0:
            w = [(0, _leaf(rnd, 1))]  # position 0 alone: the next call's position 1 meets it as a stored sibling
        elif ci == 1:
            w = [(1, _leaf(rnd, 0))] + _prefix(rnd, 2**32 - 1, 2**31, 2**32 - 2, pool[6], pool[7])
        else:
            w = [(pool[7] ^ 1, _leaf(rnd, 1))] + _prefix(rnd, pool[8], 0, 2**31, 2**32 - 1, 2**32 - 2)
        w = w[:n]
        while len(w) < n:
            p = rnd.choice(pool) if rnd.random() < 0.8 else rnd.getrandbits(32)
            w.append((p, 0 if rnd.random() < 0.03 else _leaf(rnd, len(w))))
        calls.append(w)
    return calls


def _seq_depth4(n):
    rnd = random.Random(4)
    w = _prefix(rnd, 5, 8, 12, 3, 15)
    return w + [(rnd.randrange(16), _leaf(rnd, i)) for i in range(n - len(w))]


# name -> (depth, [calls]); a call is a list of (position, raw leaf)
SEQUENCES = {
    "d3": (3, [_seq_depth3()]),
    "d3_split": (3, [_seq_depth3()[:6], _seq_depth3()[6:]]),   # the same writes as two calls
    "d32_cpu": (32, _seq_depth32((1, 12, 17), 32)),
    "d32_gpu": (32, _seq_depth32((1, 127, 130), 33)),
    "d32_switch": (32, _seq_depth32((128, 129), 34)),         # the last one-workgroup size, the first launch-per-level one
    "d4": (4, [_seq_depth4(1100)]),
}


def properties(depth, calls) -> dict:
    """which of the cases the tests rely on a sequence shows (brute force)"""
    got = dict.fromkeys(("same_twice", "pair_lr", "pair_rl", "zero_leaf", "over_r", "stored_from_earlier_call"), False)
    written = set()
    for call in calls:
        for k, (p, v) in enumerate(call):
            if k:
                q = call[k - 1][0]
                got["same_twice"] |= q == p
                got["pair_lr"] |= q == p ^ 1 and p & 1 == 1
                got["pair_rl"] |= q == p ^ 1 and p & 1 == 0
            got["zero_leaf"] |= v == 0
            got["over_r"] |= v >= R
            # a sibling node no earlier write of this call lies under, stored by an earlier call
            for lv in range(depth):
                sib = (p >> lv) ^ 1
                if not any((q >> lv) == sib for q, _ in call[:k]) and any((q >> lv) == sib for q in written):
                    got["stored_from_earlier_call"] = True
        written |= {p for p, _ in call}
    return got


class OneByOneTree(Z.SparseTree):
    """SparseTree as it is, except that a subtree with no written leaf below it
    reads as SparseTree's own zero[level] without being walked (SparseTree
    recurses to the leaves: 2^32 of them at depth 32)."""

    def __init__(self, depth):
        super().__init__(depth)
        self._occupied = set()

    def set(self, index, leaf):
        super().set(index, leaf)
        self._occupied.update((lv, index >> lv) for lv in range(self.depth + 1))

    def _node(self, level, index):
        if (level, index) not in self._occupied:
            return self.zero[level]
        return super()._node(level, index)


@functools.lru_cache(maxsize=None)
def run_one_by_one(name: str) -> dict:
    """SparseTree written one leaf at a time: per call, per write (siblings,
    replaced leaf, root after); then the final tree"""
    depth, calls = SEQUENCES[name]
    tree = OneByOneTree(depth)
    out = []
    for call in calls:
        res = []
        for p, v in call:
            sib, _ = tree.path(p)
            old = tree.leaves.get(p, 0)
            tree.set(p, v % R)
            res.append((sib, old, tree.root()))
        out.append(res)
    return {"depth": depth, "calls": out, "tree": tree}


# ----------------------------------------------------- the sequencer's witness
def account_id(tag: int, position: int, depth: int) -> bytes:
    """a 32-byte id whose leading `depth` bits are `position`"""
    return ((position << (32 - depth)) | (tag & ((1 << (32 - depth)) - 1))).to_bytes(4, "big") + bytes([tag] * 28)


def pubkey_of(aid: bytes) -> int:
    return int.from_bytes(aid, "big") % R  # account_tree.rs:188-192


def witness_oracle(depth, accounts, batches, max_transfers, max_withdrawals):
    """build_witness_with_proofs restated: accounts = [(id, balance, nonce)]
    inserted first, one at a time; batches = [{"batch_id", "transfers":
    [(sender, receiver, amount, signature)], "withdrawals": [(sender,
    l1_recipient, amount, signature)]}].  The tree is walked transfer by
    transfer: sender path, sender update, receiver path against the new root,
    receiver update; then the withdrawals.  -> (dicts, the tree)"""
    tree = Z.SparseTree(depth)
    state = {}
    for aid, bal, nonce in accounts:
        pos = int.from_bytes(aid[:4], "big") >> (32 - depth)
        state[aid] = [pubkey_of(aid), bal, nonce, pos]
        tree.set(pos, Z.account_leaf(pubkey_of(aid), bal, nonce))
    empty_sh = Z.mimc_hash(0, 0)
    out = []
    for b in batches:
        bid = b["batch_id"]
        pre = tree.root()
        ts, ws, tx_data, wd_data = [], [], [], []
        for s, r, amount, sig in b.get("transfers", [])[:max_transfers]:
            spk, sbal, snonce, spos = state[s]
            spath, sidx = tree.path(spos)
            state[s][1:3] = [max(0, sbal - amount), snonce + 1]
            tree.set(spos, Z.account_leaf(spk, state[s][1], state[s][2]))
            rpk, rbal, rnonce, rpos = state[r]
            rpath, ridx = tree.path(rpos)
            state[r][1] = rbal + amount
            tree.set(rpos, Z.account_leaf(rpk, state[r][1], rnonce))
            ts.append({"sender_pubkey": spk, "sender_balance": sbal, "sender_nonce": snonce,
                       "sender_path": spath, "sender_path_indices": sidx,
                       "receiver_pubkey": rpk, "receiver_balance": rbal, "receiver_nonce": rnonce,
                       "receiver_path": rpath, "receiver_path_indices": ridx,
                       "amount": amount, "signature": sig, "is_valid": True})
            tx_data.append((spk, rpk, amount, snonce))
        for s, l1, amount, sig in b.get("withdrawals", [])[:max_withdrawals]:
            spk, sbal, snonce, spos = state[s]
            spath, sidx = tree.path(spos)
            state[s][1:3] = [max(0, sbal - amount), snonce + 1]
            tree.set(spos, Z.account_leaf(spk, state[s][1], state[s][2]))
            ws.append({"sender_pubkey": spk, "sender_balance": sbal, "sender_nonce": snonce,
                       "sender_path": spath, "sender_path_indices": sidx,
                       "l1_recipient": l1, "amount": amount, "signature": sig, "is_valid": True})
            wd_data.append((spk, l1, amount))
        wd_acc = Z.mimc_hash(5, bid)
        for spk, l1, amount in wd_data:
            wd_acc = Z.mimc_hash(wd_acc, Z.mimc_hash(l1, amount, spk))
        out.append({"pre_state_root": pre, "post_state_root": tree.root(), "pre_shielded_root": empty_sh,
                    "post_shielded_root": empty_sh, "withdrawal_root": Z.mimc_hash(wd_acc, len(ws)),
                    "batch_hash": Z.batch_hash_host(bid, transfers=tx_data, withdrawals=wd_data), "batch_id": bid,
                    "num_transfers": len(ts), "num_withdrawals": len(ws), "num_shielded": 0,
                    "transfers": ts, "withdrawals": ws, "shielded": []})
    return out, tree
