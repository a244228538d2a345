"""Dev tool: measure the nullifier set and ShieldedPool.settle.

    python tools/nullifier_set.py [--out profiles/nullifier_set/measure.jsonl] [--reps 5]
                                  [--preload 20 22] [--skip-settle]

Wall time of whole calls (host arrays in, results on the host out), median and
minimum over --reps after one warm-up call.

  spend   2^10 .. 2^16 fresh keys, two a transfer, into a set that already
          holds 2^20 and 2^22 keys; every repeat spends other fresh keys, so
          every call accepts and inserts all of its keys.  Beside it the same
          piles through a Python set of bytes holding the same keys: what a
          user of DeviceNoteTree does today (first one wins, in order).
  settle  256 transfers of compressed proofs through ShieldedPool.settle, and
          the same pile by hand: verify_many_encoded, the Python set loop,
          one DeviceNoteTree.append.  Proof verification does not depend on the
          circuit's size, so the pile is proven over a depth-10 tree (shape
          (10, 10, 2): 512 notes in, 512 out fill its 1,024 leaves); every
          repeat runs on a fresh pool that holds the same 512 notes.

One raw JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zelana_amd import gpu  # noqa: E402


def stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "reps": len(ts)}


def py_spend(stored: set, keys: list, per_tx: int):
    """first one wins, in order, over a Python set; -> accepted transfers"""
    accepted = 0
    for t in range(0, len(keys), per_tx):
        mine = keys[t:t + per_tx]
        if any(k in stored for k in mine) or len(set(mine)) != per_tx:
            continue
        stored.update(mine)
        accepted += 1
    return accepted


def measure_spend(ctx, emit, rng, log2_preload, reps):
    n0 = 1 << log2_preload
    sizes = [1 << e for e in range(10, 17)]
    dev = gpu.NullifierSetDevice(ctx, n0 + (reps + 1) * sum(sizes))
    base = np.frombuffer(rng.bytes(32 * n0), np.uint8).reshape(n0, 32)
    t0 = time.perf_counter()
    v, _, rounds = dev.load(base)
    emit({"what": "load", "keys": n0, "ms": 1e3 * (time.perf_counter() - t0), "rounds": rounds,
          "accepted": v.count(0)})
    stored = {base[i].tobytes() for i in range(n0)}
    for n in sizes:
        piles = [np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32) for _ in range(reps + 1)]
        ts, acc = [], []
        for i, p in enumerate(piles):
            t0 = time.perf_counter()
            v, _, rounds = dev.spend(p, 2)
            ts.append(time.perf_counter() - t0)
            acc.append(v.count(0))
        emit({"what": "spend", "stored": n0, "keys": n, "per_tx": 2, **stats(ts[1:]), "rounds": rounds,
              "accepted_per_call": acc[-1], "count_after": dev.count})
        ts, acc = [], []
        for p in piles:
            as_bytes = [p[i].tobytes() for i in range(n)]  # the form a Python user holds them in: not timed
            t0 = time.perf_counter()
            acc.append(py_spend(stored, as_bytes, 2))
            ts.append(time.perf_counter() - t0)
        emit({"what": "python_set", "stored": n0, "keys": n, "per_tx": 2, **stats(ts[1:]), "accepted_per_call": acc[-1]})
    probes = np.concatenate([base[:1 << 15], np.frombuffer(rng.bytes(32 << 15), np.uint8).reshape(-1, 32)])
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        got = dev.contains(probes)
        ts.append(time.perf_counter() - t0)
    assert got == [True] * (1 << 15) + [False] * (1 << 15)
    emit({"what": "contains", "stored": dev.count, "keys": 1 << 16, **stats(ts[1:])})
    dev.close()


def measure_settle(ctx, emit, reps, ntx=256, depth=10):
    from zelana_amd import shielded as S, shielded_pool as SP
    fmt = gpu.PROOF_ARK_COMPRESSED
    t0 = time.perf_counter()
    sp = S.ShieldedProver(ctx, (depth, depth, 2), seed=0)
    emit({"what": "keygen", "shape": [depth, depth, 2], "s": time.perf_counter() - t0})

    def b32(i, tag):
        return (i * 0x9E3779B97F4A7C15 + tag).to_bytes(32, "little")

    specs = [(1000 + i, b32(i, 1), b32(i, 2), i) for i in range(2 * ntx)]
    outs = [[S.OutputNote(1500 + 2 * t, b32(t, 3), b32(t, 4)), S.OutputNote(499 + 2 * t, b32(t, 5), b32(t, 6))]
            for t in range(ntx)]

    def fresh_pool():
        pool = SP.ShieldedPool(ctx, sp, depth=depth, capacity=1 << depth, nullifier_capacity=1 << 12, empty_leaf=0)
        return pool, pool.tree.spend_notes(specs)

    pool, notes = fresh_pool()
    ts_ = S.honest_many(pool.tree.hasher, [notes[2 * t:2 * t + 2] for t in range(ntx)], outs, tree=pool.tree)
    pool.close()
    t0 = time.perf_counter()
    proofs = sp.prove_many(ts_, range(100, 100 + ntx))
    emit({"what": "prove_many", "nb": ntx, "s": time.perf_counter() - t0})
    raws = b"".join(p.compressed() for p in proofs)
    pubs = [[t.merkle_root] + list(t.nullifiers) + list(t.commitments) + [S._b32(t.fee)] for t in ts_]
    ts, by_hand = [], []
    for _ in range(reps + 1):
        pool, _ = fresh_pool()
        t0 = time.perf_counter()
        got = pool.settle(fmt, raws, pubs)
        ts.append(time.perf_counter() - t0)
        assert all(s.accepted for s in got) and pool.tree.next_position == 4 * ntx
        pool.close()
        # by hand: the same pile over a DeviceNoteTree and a Python set
        pool, _ = fresh_pool()
        spent = set()
        t0 = time.perf_counter()
        ints = [[int.from_bytes(v, "little") for v in row] for row in pubs]
        ok = sp.verify_many_encoded(fmt, raws, ints)
        leaves = []
        for row, vals, good in zip(pubs, ints, ok):
            nfs = row[1:3]
            if not good or not pool.tree.is_valid_root(vals[0]) or any(k in spent for k in nfs) or nfs[0] == nfs[1]:
                continue
            spent.update(nfs)
            leaves += vals[3:5]
        pool.tree.append(leaves)
        by_hand.append(time.perf_counter() - t0)
        assert len(leaves) == 2 * ntx
        pool.close()
    emit({"what": "settle", "ntx": ntx, "depth": depth, "fmt": "compressed", **stats(ts[1:])})
    emit({"what": "by_hand_verify_set_append", "ntx": ntx, "depth": depth, "fmt": "compressed", **stats(by_hand[1:])})
    sp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nullifier_set", "measure.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--preload", type=int, nargs="*", default=[20, 22], help="log2 of the keys stored beforehand")
    ap.add_argument("--skip-settle", action="store_true")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rng = np.random.default_rng(13)
    ctx = gpu.Context(0)
    with open(a.out, "a") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(rec, flush=True)

        for e in a.preload:
            measure_spend(ctx, emit, rng, e, a.reps)
        if not a.skip_settle:
            measure_settle(ctx, emit, a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
