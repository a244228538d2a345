"""Dev tool: the batched Poseidon hash and the GPU-resident note tree at the
sizes a sequencer sees.  Prints one JSON line per figure.

    python tools/note_tree.py [hash] [append] [paths] [rebuild] [baseline]   # default: all

Every figure is the median of REPS (11) calls after a warm call, with the
spread (min, max) and the raw times ("raw").  "ms" is the whole call as a
caller sees it (upload, kernels, download, on the context stream); "kernel_ms"
is the library's own timer around the kernels alone.
  hash      hash_many of 2^20 pairs and of 2^20 four-tuples, hashes per second
            (the lane-per-hash kernel), and of 1 and 512 three-tuples under both
            mappings
  append    into a tree of capacity 2^20 that already holds 2^19 leaves: append
            of 1, 512 and 2^16 leaves, with and without per-insertion roots (a
            fresh such tree whenever the next append would not fit), under both
            mappings, alternated: "default" = the library's choice (a quad of
            lanes per hash where a launch has at most 16384 hashes), "lanes" =
            one lane per hash everywhere (ZKMI_DEBUG_NOTE_TREE_NO_QUAD=1)
  paths     paths of 512 random positions of that tree
  rebuild   one append of 2^20 leaves into an empty tree
  baseline  the same hash loop of the host-compiled header
            (tests/host/note_tree_check.cpp, g++ -O2, one thread) on this
            machine's CPU: NOT the reference's Rust, which is not built here
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("NT_REPS", "11"))
CAP = 1 << 20


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "raw": [round(x, 4) for x in xs]}


def timed(ctx, fn, names):
    """(wall ms, {timer: kernel ms}) of one call"""
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    fn()
    ms = (time.perf_counter() - t0) * 1e3
    k = {n: ctx.profile_get(n)[0] for n in names}
    ctx.profile(False)
    return ms, k


def rand_words(rng, n, width):
    """n x width field elements as any 256-bit values"""
    return rng.integers(0, 2**64, size=(n, 4 * width), dtype=np.uint64)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def bench_hash(ctx, h, rng):
    for arity in (2, 4):
        ins = rand_words(rng, CAP, arity)
        runs = [timed(ctx, lambda: h.hash_many(ins, arity), ["poseidon_hash_many"]) for _ in range(REPS + 1)][1:]
        ms, km = [r[0] for r in runs], [r[1]["poseidon_hash_many"] for r in runs]
        emit(what="hash_many", n=CAP, arity=arity, reps=REPS, ms=stats(ms), kernel_ms=stats(km),
             hashes_per_s=round(CAP / statistics.median(ms) * 1e3), kernel_hashes_per_s=round(
                 CAP / statistics.median(km) * 1e3))


def half_full(ctx, h, rng):
    from zelana_amd import gpu
    t = gpu.NoteTreeDevice(ctx, h, 32, CAP, 0)
    t.append(rand_words(rng, CAP // 2, 1), want_roots=False)
    return t


def bench_append(ctx, hs, rng):
    """hs: {"default": the library's choice of mapping, "lanes": a lane per hash everywhere}"""
    names = ["note_tree_append", "note_tree_roots"]
    trees = {m: half_full(ctx, h, rng) for m, h in hs.items()}
    for n in (1, 512, 1 << 16):
        leaves = rand_words(rng, n, 1)
        res = {(m, want): [] for m in hs for want in (False, True)}
        for rep in range(REPS + 1):
            for key in res:  # alternated, so all four see the same session
                m, want = key
                if trees[m].next_position + n > CAP:
                    trees[m].close()
                    trees[m] = half_full(ctx, hs[m], rng)
                run = timed(ctx, lambda: trees[m].append(leaves, want_roots=want), names)
                if rep:
                    res[key].append(run)
        for (m, want), runs in res.items():
            emit(what="append", mapping=m, n=n, per_insertion_roots=want, capacity=CAP, held=CAP // 2, reps=REPS,
                 ms=stats([r[0] for r in runs]),
                 kernel_ms=stats([r[1]["note_tree_append"] + r[1]["note_tree_roots"] for r in runs]))
    trees.pop("lanes").close()
    return trees["default"]


def bench_hash_short(ctx, hs, rng):
    """a short hash_many (what commit_many of one block's notes is) under both mappings"""
    for n in (1, 512):
        ins = rand_words(rng, n, 3)
        res = {m: [] for m in hs}
        for rep in range(REPS + 1):
            for m, h in hs.items():
                run = timed(ctx, lambda: h.hash_many(ins, 3), ["poseidon_hash_many"])
                if rep:
                    res[m].append(run)
        for m, runs in res.items():
            emit(what="hash_many", mapping=m, n=n, arity=3, reps=REPS, ms=stats([r[0] for r in runs]),
                 kernel_ms=stats([r[1]["poseidon_hash_many"] for r in runs]))


def bench_paths(ctx, t, rng):
    pos = rng.integers(0, t.next_position, size=512, dtype=np.uint64)
    runs = [timed(ctx, lambda: t.paths(pos), ["note_tree_paths"]) for _ in range(REPS + 1)][1:]
    emit(what="paths", n=512, held=t.next_position, reps=REPS, ms=stats([r[0] for r in runs]),
         kernel_ms=stats([r[1]["note_tree_paths"] for r in runs]))


def bench_rebuild(ctx, h, rng):
    from zelana_amd import gpu
    leaves = rand_words(rng, CAP, 1)
    runs = []
    for _ in range(REPS + 1):
        t = gpu.NoteTreeDevice(ctx, h, 32, CAP, 0)
        runs.append(timed(ctx, lambda: t.append(leaves, want_roots=False), ["note_tree_append"]))
        t.close()
    runs = runs[1:]
    emit(what="rebuild", n=CAP, reps=REPS, ms=stats([r[0] for r in runs]),
         kernel_ms=stats([r[1]["note_tree_append"] for r in runs]))


def bench_baseline():
    """the header's own sponge on one CPU thread (g++ -O2): a chain of dependent hashes"""
    from zelana_amd.shielded import shielded_params
    p = shielded_params()
    table = [c for row in p["ark"] for c in row] + [c for row in p["mds"] for c in row]
    count = int(os.environ.get("NT_BASELINE_HASHES", "20000"))
    with tempfile.TemporaryDirectory() as d:
        exe, script = os.path.join(d, "note_tree_check"), os.path.join(d, "script.txt")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "note_tree_check.cpp")],
                       check=True, capture_output=True)
        with open(script, "w") as f:
            f.write(f"C {p['full']} {p['partial']} " + " ".join(int(c).to_bytes(32, "little").hex() for c in table))
            f.write("\n" + "\n".join(f"B {count} {a}" for a in (2, 4) for _ in range(REPS + 1)) + "\n")
        out = subprocess.run([exe, script], check=True, capture_output=True, text=True).stdout.split("\n")
    rates = [float(line.split()[1]) for line in out if line.startswith("b ")]
    for k, arity in enumerate((2, 4)):
        r = rates[k * (REPS + 1) + 1:(k + 1) * (REPS + 1)]
        emit(what="baseline_host_header_one_thread_O2", arity=arity, hashes=count, reps=REPS,
             hashes_per_s=stats(r))


def main():
    which = set(sys.argv[1:]) or {"hash", "append", "paths", "rebuild", "baseline"}
    rng = np.random.default_rng(2024)
    if which - {"baseline"}:
        from zelana_amd import gpu, shielded as S
        ctx = gpu.Context(0)
        h = S.shielded_hasher(ctx)
        os.environ["ZKMI_DEBUG_NOTE_TREE_NO_QUAD"] = "1"  # read by zkmi_poseidon_create
        h_lanes = S.shielded_hasher(ctx)
        del os.environ["ZKMI_DEBUG_NOTE_TREE_NO_QUAD"]
        hs = {"default": h, "lanes": h_lanes}
        if "hash" in which:
            bench_hash(ctx, h, rng)
            bench_hash_short(ctx, hs, rng)
        t = None
        if "append" in which:
            t = bench_append(ctx, hs, rng)
        if "paths" in which:
            t = t or half_full(ctx, h, rng)
            bench_paths(ctx, t, rng)
        if t is not None:
            t.close()
        if "rebuild" in which:
            bench_rebuild(ctx, h, rng)
        h.close()
        h_lanes.close()
        ctx.close()
    if "baseline" in which:
        bench_baseline()


if __name__ == "__main__":
    main()
