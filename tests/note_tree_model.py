"""Plain-Python models shared by the note-tree tests (CPU and GPU): the
reference's MerkleTree one leaf at a time, a level-by-level rebuild, and the
inputs both suites use.  Every hash is shielded.sponge_hash (1.25 ms each), so
results are cached per process."""
import functools
import random

import numpy as np

from zelana_amd.r1cs import R
from zelana_amd.shielded import shielded_params, sponge_hash

# the values at and around the modulus, and the largest 256-bit value
SPECIALS = [0, 1, R - 1, R, R + 1, 2**256 - 1]


@functools.lru_cache(maxsize=None)
def _h(xs):
    return sponge_hash(*xs)


def H(*xs) -> int:
    """sponge_hash of the values mod r (what Fr::from_le_bytes_mod_order feeds it)"""
    return _h(tuple(int(x) % R for x in xs))


def fe_hex(v: int) -> str:
    return int(v).to_bytes(32, "little").hex()


def hex_fe(s: str) -> int:
    return int.from_bytes(bytes.fromhex(s), "little")


def words(vals) -> np.ndarray:
    """any 256-bit ints -> (n, 4) u64, little-endian, NOT reduced"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, np.uint64).reshape(-1, 4).copy()


def ints(arr) -> list:
    a = np.ascontiguousarray(arr, np.uint64).reshape(-1, 4)
    return [int.from_bytes(row.tobytes(), "little") for row in a]


def params_table() -> list:
    """the constants in the order of a kind-9 op's table: ark[r][i], then mds[i][j]"""
    p = shielded_params()
    return [c % R for row in p["ark"] for c in row] + [c % R for row in p["mds"] for c in row]


def hash_inputs(arity: int, n: int, seed: int) -> list:
    """n tuples of 256-bit values; the first len(SPECIALS) carry one special
    value each, in a position that moves with the index"""
    rng = random.Random(1000 * arity + seed)
    out = []
    for i in range(n):
        t = [rng.getrandbits(256) if rng.random() < 0.5 else rng.randrange(R) for _ in range(arity)]
        if i < len(SPECIALS):
            t[i % arity] = SPECIALS[i]
        out.append(tuple(t))
    return out


def leaf_values(n: int, seed: int) -> list:
    """leaves as a client may send them: mostly < r, every fifth one any 256-bit
    value, the specials among the first"""
    rng = random.Random(seed)
    out = [rng.getrandbits(256) if i % 5 == 4 else rng.randrange(R) for i in range(n)]
    for i, v in zip(range(1, n, 3),(R - 1, R, R + 1, 2**256 - 1, 2 * R + 5)):
        out[i] = v
    return out


def empty_chain(empty_leaf: int, depth: int) -> list:
    e = [empty_leaf % R]
    for _ in range(depth):
        e.append(H(e[-1], e[-1]))
    return e


class OneByOneTree:
    """MerkleTree of sdk/privacy/src/merkle.rs: insert = insert_at(next_index)."""

    def __init__(self, depth: int, empty_leaf: int):
        self.depth, self.empty = depth, empty_chain(empty_leaf, depth)
        self.nodes, self.next, self.root = {}, 0, self.empty[depth]

    def insert(self, leaf: int) -> int:
        pos = idx = self.next
        cur = self.nodes[(0, pos)] = leaf % R
        for level in range(self.depth):
            sib = self.nodes.get((level, idx ^ 1), self.empty[level])
            cur = H(sib, cur) if idx & 1 else H(cur, sib)
            idx >>= 1
            self.nodes[(level + 1, idx)] = cur
        self.root = cur
        self.next += 1
        return pos

    def path(self, pos: int) -> list:
        return [self.nodes.get((level, (pos >> level) ^ 1), self.empty[level]) for level in range(self.depth)]


def run_one_by_one(depth: int, empty_leaf: int, leaves) -> dict:
    """every per-insertion root, the final root and every leaf's path under it"""
    t = OneByOneTree(depth, empty_leaf)
    roots = []
    for v in leaves:
        t.insert(v)
        roots.append(t.root)
    return {"roots": roots, "root": t.root, "paths": [t.path(i) for i in range(len(leaves))],
            "leaves": [v % R for v in leaves], "empty": t.empty}


class RebuiltTree:
    """The tree of `leaves` built level by level, each node hashed once."""

    def __init__(self, depth: int, empty_leaf: int, leaves):
        self.depth, self.empty = depth, empty_chain(empty_leaf, depth)
        self.levels = [[v % R for v in leaves]]
        for level in range(depth):
            cur = self.levels[-1]
            self.levels.append([H(cur[2 * i], cur[2 * i + 1] if 2 * i + 1 < len(cur) else self.empty[level])
                                for i in range((len(cur) + 1) // 2)])
        self.root = self.levels[depth][0] if leaves else self.empty[depth]

    def node(self, level: int, idx: int) -> int:
        lv = self.levels[level]
        return lv[idx] if idx < len(lv) else self.empty[level]

    def path(self, pos: int) -> list:
        return [self.node(level, (pos >> level) ^ 1) for level in range(self.depth)]

    def root_after(self, k: int) -> int:
        """the root when leaf k had just been inserted: the frontier fold (a
        left sibling is final, a right one was still empty)"""
        cur, idx = self.levels[0][k], k
        for level in range(self.depth):
            cur = H(self.node(level, idx - 1), cur) if idx & 1 else H(cur, self.empty[level])
            idx >>= 1
        return cur


# the append sequences of the issue: (depth, capacity, appends)
SEQUENCES = [(3, 8, (1, 2, 5)), (32, 64, (1, 2, 5, 29))]
