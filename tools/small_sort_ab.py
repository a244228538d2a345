"""Dev tool: time the smallest MSMs the library runs, the ones whose windows lie
below 12 and whose sort is the round-4 radix sort (k_rs_*), for an A/B of
another sort for them (profiles/one_small_sort/: the counting sort, measured
and not adopted).  Run it from the checkout of each side, alternating the two
in one session.  One JSON line per shape.

    python tools/small_sort_ab.py run TAG [big]    # the gate shapes (or the pinned-window 2^20 ones)
    python tools/small_sort_ab.py compare FILE...  # same shape and seed -> same result in every line; exits 1 if not

Shapes, all with automatic windows:
  A  plain G1 MSM, n = 512, 2^10, 2^12, 2^13; uniform and 0/1 witness-like scalars
  B  full-table MSM over 1,024 bases, G1 and G2
  C  msm_batch of 16 plain vectors of 2^13
`big`: a pinned window 8 or 11 at n = 2^20 (what only tools do).
Every shape is warmed, then timed call by call (each call ends in a wait on
its result) with the profiler off until the window is >= SS_WINDOW seconds
(default 0.6); `ms` is the median call.  A short profiled loop after it gives
`sort_ms`, the library's msm_sort timer per call.  Inputs are seeded, bases
and uniform scalars generated on the device; `res` is the result's SHA-256.
"""
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW = float(os.environ.get("SS_WINDOW", "0.6"))


def measure(ctx, fn, warm, min_reps):
    for _ in range(warm):
        r = fn()
    ts, t_end = [], time.perf_counter() + WINDOW
    while len(ts) < min_reps or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    ctx.profile(True)
    ctx.profile_reset()
    k = max(3, min(50, len(ts)))
    for _ in range(k):
        fn()
    ctx.profile(False)
    t, cnt = ctx.profile_get("msm_sort")
    return r, dict(ms=round(1e3 * statistics.median(ts), 5), reps=len(ts), window_s=round(sum(ts), 3),
                   sort_ms=round(t / k, 5), sorts_per_call=cnt / k)


def witness_bits(seed, n):
    sc = np.zeros((n, 4), np.uint64)
    sc[:, 0] = np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint64)
    return sc


def scalars(ctx, kind, seed, n):
    from zelana_amd.gpu import DeviceBuffer
    if kind == "uniform":
        return ctx.scalars_generate(seed, n)
    d = DeviceBuffer(ctx, n * 32)
    d.upload(witness_bits(seed, n))
    return d


def run(tag, big):
    from zelana_amd.gpu import Context
    ctx = Context(0)
    out = []

    def emit(shape, r, m, **kw):
        line = dict(tag=tag, shape=shape, **kw, **m, res=hashlib.sha256(np.ascontiguousarray(r).tobytes()).hexdigest())
        print(json.dumps(line), flush=True)

    if big:
        n = 1 << 20
        b = ctx.bases_generate(1020, n)
        for c in (8, 11):
            for kind in ("uniform", "witness"):
                d = scalars(ctx, kind, 20, n)
                ctx.set_window(c)
                r, m = measure(ctx, lambda: ctx.msm(b, d), 2, 5)
                ctx.set_window(0)
                emit(f"big_c{c}_{kind}", r, m, n=n, window=c)
                d.free()
        ctx.close()
        return
    bases = ctx.bases_generate(1020, 1 << 13)
    for n in (512, 1 << 10, 1 << 12, 1 << 13):
        for kind in ("uniform", "witness"):
            d = scalars(ctx, kind, 20 + n, n)
            r, m = measure(ctx, lambda: ctx.msm_device_n(bases, d, n), 50, 200)
            emit(f"A_plain_g1_{n}_{kind}", r, m, n=n)
            d.free()
    for g2 in (False, True):
        t = ctx.bases_generate(1024, 1024, g2)
        info = t.precompute()
        d = scalars(ctx, "uniform", 31, 1024)
        r, m = measure(ctx, lambda: ctx.msm_device_n(t, d, 1024), 50, 200)
        emit(f"B_table_1024_{'g2' if g2 else 'g1'}", r, m, n=1024, window=info[1])
        d.free()
    n, nb = 1 << 13, 16
    d = scalars(ctx, "uniform", 47, n * nb)
    r, m = measure(ctx, lambda: ctx.msm_batch(bases, d, n, nb, n * 32), 20, 100)
    emit("C_batch16_plain_8192", r, m, n=n, nb=nb)
    ctx.close()


def compare(files):
    seen, bad = {}, 0
    for f in files:
        for line in open(f):
            if not line.startswith("{"):
                continue
            j = json.loads(line)
            first = seen.setdefault(j["shape"], (j["tag"], j["res"]))
            if first[1] != j["res"]:
                print(f"MISMATCH {j['shape']}: {first[0]} {first[1][:16]} != {j['tag']} {j['res'][:16]}")
                bad += 1
    print(f"compared {len(seen)} shapes: {'all equal' if not bad else str(bad) + ' mismatches'}")
    return 1 if bad or not seen else 0


if __name__ == "__main__":
    if sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2:]))
    run(sys.argv[2], len(sys.argv) > 3 and sys.argv[3] == "big")
