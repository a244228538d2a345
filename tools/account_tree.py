"""Dev tool: measure the batched MiMC hash and the account tree.

    python tools/account_tree.py [--out profiles/account_tree/measure.jsonl] [--reps 7]

Wall time of whole calls (host pointers in, results on the host out), median
and minimum over --reps after one warm-up: hash_many, apply at K = 1, 20, 512,
4096 and 2^16 on a depth-32 tree, and paths.  The comparison is ONE host thread
of libzelana_prover.so's zp_mimc_permute walking the same writes one at a time
(two permutations a level, the constant first permutation of hash_2 folded),
through ctypes: a native host loop, not Python's hash.  One raw JSON line per
measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zelana_amd import gpu, zbatch as Z  # noqa: E402
from zelana_amd.r1cs import R  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "reps": reps}


def host_walk(positions, leaves, depth):
    """one host thread, zp_mimc_permute, one write at a time over a dict of nodes"""
    L = Z._native_mimc()
    if L is None:
        return None
    buf, key, out = np.zeros(4, np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint64)

    def perm(x):
        buf[:] = Z._limbs(x)
        L.zp_mimc_permute(buf.ctypes.data, key.ctypes.data, out.ctypes.data)
        return Z._int(out)

    p2 = perm(2)
    zero = [0]
    for _ in range(depth):
        zero.append(perm((perm((p2 + zero[-1]) % R) + zero[-1]) % R))
    nodes = {}
    t0 = time.perf_counter()
    for pos, leaf in zip(positions, leaves):
        cur = leaf
        nodes[(0, pos)] = cur
        for lv in range(depth):
            i = pos >> lv
            sib = nodes.get((lv, i ^ 1), zero[lv])
            a, b = (sib, cur) if i & 1 else (cur, sib)
            cur = perm((perm((p2 + a) % R) + b) % R)
            nodes[(lv + 1, i >> 1)] = cur
    return time.perf_counter() - t0, cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "account_tree", "measure.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rng = np.random.default_rng(12)
    ctx = gpu.Context(0)
    h = gpu.MimcHasher(ctx)
    depth = 32
    with open(a.out, "a") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(rec)

        for arity in (2, 4):
            for n in (1, 1024, 1 << 16, 1 << 20):
                ins = rng.integers(0, 2**64, size=(n, 4 * arity), dtype=np.uint64)
                emit({"what": "mimc_hash_many", "arity": arity, "n": n, **timed(lambda: h.hash_many(ins, arity), a.reps)})
        tree = gpu.AccountTreeDevice(ctx, h, depth, 4 * (1 << 16) * (depth + 1))
        for K in (1, 20, 512, 4096, 1 << 16):
            pos = rng.integers(0, 2**32, size=K, dtype=np.uint64)
            lv = rng.integers(0, 2**64, size=(K, 4), dtype=np.uint64)
            lv[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)  # below r: the host walk takes the same values
            rec = {"what": "account_tree_apply", "depth": depth, "K": K, **timed(lambda: tree.apply(pos, lv), a.reps),
                   "nodes_stored": tree.node_count}
            emit(rec)
            if K <= 512:
                fresh = gpu.AccountTreeDevice(ctx, h, depth, 2 * K * (depth + 1))
                root = Z._int(fresh.apply(pos, lv)[2][-1])
                fresh.close()
                got = host_walk([int(p) for p in pos], [Z._int(x) for x in lv], depth)
                if got is None:
                    emit({"what": "host_walk_one_thread_zp_mimc_permute", "K": K, "unmeasured": "libzelana_prover.so not built"})
                else:
                    emit({"what": "host_walk_one_thread_zp_mimc_permute", "depth": depth, "K": K, "ms": 1e3 * got[0],
                          "root_equals_gpu": got[1] == root})
        for n in (20, 4096):
            pos = rng.integers(0, 2**32, size=n, dtype=np.uint64)
            emit({"what": "account_tree_paths", "depth": depth, "n": n, **timed(lambda: tree.paths(pos), a.reps)})
        tree.close()
    h.close()
    ctx.close()


if __name__ == "__main__":
    main()
