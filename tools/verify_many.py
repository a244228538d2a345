"""Dev tool: batched verification (zkmi_groth16_verify_many) against the loop
of zkmi_groth16_verify a caller has without it, in one run on the same proofs.
Prints one JSON line per nb.

    python tools/verify_many.py [nb ...]         # default 1 64 1024

Proofs: square_circuit(x) for 64 distinct x under one key (GPU keygen), tiled
to nb (the weights differ per position, so a repeated proof is its own lane's
work).  Per nb: the batched call (all valid, weights drawn by the library),
warmed, then the median of VM_REPS calls (default 11) with the profiler off;
then three more calls with it on for the two kernels' times (zkmi_profile_get
verify_prepare / verify_miller); then ONE timed loop of zkmi_groth16_verify
over the same nb proofs (capped at VM_HOST_CAP proofs, default 1024, and
scaled).
`one_bad_ms`: the batched call with one proof's input changed (bisection).

    python tools/verify_many.py --each [nb ...]

Per nb, on the same proofs: zkmi_groth16_verify_each on the all-valid batch
and on the all-bad batch (every input + 1), each warmed and the median of
VM_REPS calls with the profiler off (`*_spread_ms` = max - min of those
calls); its four kernel times from three further calls with the profiler on;
verify_many under the probe budget VM_BUDGET (default 1) on the all-bad batch,
the same way; verify_many without a budget on that batch, timed ONCE (about
2 nb probes); one bad proof without a budget (`probe_ms` = the extra time per
extra final exponentiation, the figure the crossover is taken from); the host
loop as above.  Against a library without verify_each (ZKMI_LIB pointing at an
older build) only the unbudgeted and host figures are reported.

    python tools/verify_many.py --encoded FMT [nb ...]

FMT: compressed, uncompressed, solana, alt_bn128 or all.  Per nb and format, on
the same proofs as wire bytes: zkmi_groth16_verify_many_encoded and
_each_encoded (decoded on the GPU) against what a caller has without them, a
host loop of zkmi_proof_decode followed by the point-taking call.  Both sides
are timed at the C ABI (buffers and pointers prepared outside the timed
region), alternated call by call in one run, warmed, median of VM_REPS calls
(`*_spread_ms` = max - min).  `decode_loop_ms`: the host loop alone.
`verify_decode_ms`: the decode kernels' time from three further calls with the
profiler on.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("VM_REPS", "11"))
HOST_CAP = int(os.environ.get("VM_HOST_CAP", "1024"))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


BUDGET = int(os.environ.get("VM_BUDGET", "1"))


def timed(fn):
    """fn warmed once, then REPS timed calls: (median ms, max - min ms, last result)"""
    out = fn()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), max(times) - min(times), out


def each_mode(ctx, vk, vkb, base, base_in, nbs):
    from zelana_amd import gpu
    from zelana_amd._lib import lib
    has_each = hasattr(lib(), "zkmi_groth16_verify_each")
    for nb in nbs:
        proofs = [base[i % 64] for i in range(nb)]
        inputs = [base_in[i % 64] for i in range(nb)]
        bad_in = [[(x[0] + 1) % R] for x in inputs]
        row = {"nb": nb, "reps": REPS, "each": has_each}
        if has_each:
            ok_ms, ok_sp, (valid, st) = timed(lambda: gpu.groth16_verify_each(ctx, vk, proofs, inputs))
            assert all(valid) and st["final_exps"] == nb
            bad_ms, bad_sp, (valid, st) = timed(lambda: gpu.groth16_verify_each(ctx, vk, proofs, bad_in))
            assert not any(valid) and st["final_exps"] == nb
            row.update({"each_valid_ms": round(ok_ms, 3), "each_valid_spread_ms": round(ok_sp, 3),
                        "each_bad_ms": round(bad_ms, 3), "each_bad_spread_ms": round(bad_sp, 3),
                        "each_per_proof_ms": round(ok_ms / nb, 4), "pairs": st["pairs"]})
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(3):
                gpu.groth16_verify_each(ctx, vk, proofs, bad_in)
            for name in ("verify_each_prepare", "verify_inputs", "verify_miller", "verify_final_exp"):
                t, n = ctx.profile_get(name)
                row[name + "_ms"] = round(t / max(n, 1), 3)
            ctx.profile(False)
            ctx.set_verify_probes(BUDGET)
            bud_ms, bud_sp, (valid, st) = timed(lambda: gpu.groth16_verify_many(ctx, vk, proofs, bad_in))
            last = gpu.groth16_verify_last(ctx)
            ctx.set_verify_probes(0)
            assert not any(valid) and st["final_exps"] <= BUDGET
            row.update({"budget": BUDGET, "budgeted_all_bad_ms": round(bud_ms, 3),
                        "budgeted_all_bad_spread_ms": round(bud_sp, 3), "budgeted_final_exps": st["final_exps"],
                        "gpu_decided": last["gpu_decided"]})
        t0 = time.perf_counter()
        valid, st = gpu.groth16_verify_many(ctx, vk, proofs, bad_in)  # no budget: timed once
        free_ms = 1e3 * (time.perf_counter() - t0)
        assert not any(valid)
        row.update({"unbudgeted_all_bad_ms": round(free_ms, 3), "unbudgeted_final_exps": st["final_exps"]})
        all_ms, _, (valid, st1) = timed(lambda: gpu.groth16_verify_many(ctx, vk, proofs, inputs))
        assert all(valid)
        one_in = [list(x) for x in inputs]
        one_in[nb // 2] = bad_in[nb // 2]
        one_ms, _, (valid, stb) = timed(lambda: gpu.groth16_verify_many(ctx, vk, proofs, one_in))
        assert valid == [i != nb // 2 for i in range(nb)]
        extra = stb["final_exps"] - st1["final_exps"]
        row.update({"verify_many_all_valid_ms": round(all_ms, 3), "one_bad_ms": round(one_ms, 3),
                    "one_bad_final_exps": stb["final_exps"],
                    "probe_ms": round((one_ms - all_ms) / extra, 3) if extra else None})
        nh = min(nb, HOST_CAP)
        t0 = time.perf_counter()
        hv = [gpu.groth16_verify(vkb, bad_in[i], *proofs[i]) for i in range(nh)]
        host_ms = 1e3 * (time.perf_counter() - t0) * nb / nh
        assert not any(hv)
        row.update({"host_loop_all_bad_ms": round(host_ms, 3), "host_loop_proofs_timed": nh})
        if has_each:
            row.update({"budgeted_vs_unbudgeted": round(free_ms / bud_ms, 2),
                        "budgeted_vs_host_loop": round(host_ms / bud_ms, 2)})
            if row["probe_ms"]:
                row["crossover_probes"] = round(ok_ms / row["probe_ms"], 1)
        print(json.dumps(row), flush=True)


def encoded_mode(ctx, vk, base, base_in, nbs, fmts):
    import ctypes

    from zelana_amd import gpu
    from zelana_amd._lib import VerifyStatsStruct, check, lib, u8p, u64p
    L = lib()
    enc = {gpu.PROOF_ARK_COMPRESSED: gpu.proof_serialize_compressed, gpu.PROOF_SOLANA_LE: gpu.proof_to_solana_bytes,
           gpu.PROOF_ALT_BN128_BE: gpu.proof_to_alt_bn128_bytes}
    names = {v: k for k, v in gpu.PROOF_FORMATS.items()}

    def uncompressed(a, b, c):  # no encoder in the library: the compressed form's x, y as given, no flags
        return b"".join(np.ascontiguousarray(p, "<u8").tobytes() for p in (a, b, c))

    for nb in nbs:
        ins = np.array([[[(base_in[i % 64][0] >> (64 * k)) & (2**64 - 1) for k in range(4)]] for i in range(nb)],
                       np.uint64)
        for fmt in fmts:
            one = [enc.get(fmt, uncompressed)(*base[i]) for i in range(64)]
            n = len(one[0])
            buf = np.frombuffer(b"".join(one[i % 64] for i in range(nb)), np.uint8)
            a, b, c = np.zeros((nb, 8), np.uint64), np.zeros((nb, 16), np.uint64), np.zeros((nb, 8), np.uint64)
            valid, mal = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
            st = VerifyStatsStruct()
            bp, ip, vp_, mp = buf.ctypes.data_as(u8p), ins.ctypes.data_as(u64p), valid.ctypes.data_as(u8p), \
                mal.ctypes.data_as(u8p)
            ap, bpp, cp = a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), c.ctypes.data_as(u64p)
            ptrs = [(ctypes.cast(buf.ctypes.data + n * i, u8p), ctypes.cast(a.ctypes.data + 64 * i, u64p),
                     ctypes.cast(b.ctypes.data + 128 * i, u64p), ctypes.cast(c.ctypes.data + 64 * i, u64p))
                    for i in range(nb)]

            def decode_loop():
                for r, pa, pb, pc in ptrs:
                    if L.zkmi_proof_decode(fmt, r, n, pa, pb, pc):
                        raise RuntimeError("a valid proof did not decode")

            calls = {
                "many_encoded": lambda: check(L.zkmi_groth16_verify_many_encoded(
                    ctx.h, vk.h, fmt, nb, bp, ip, None, vp_, mp, ctypes.byref(st))),
                "many_host_decode": lambda: (decode_loop(), check(L.zkmi_groth16_verify_many(
                    ctx.h, vk.h, nb, ip, ap, bpp, cp, None, vp_, ctypes.byref(st)))),
                "each_encoded": lambda: check(L.zkmi_groth16_verify_each_encoded(
                    ctx.h, vk.h, fmt, nb, bp, ip, vp_, mp, ctypes.byref(st))),
                "each_host_decode": lambda: (decode_loop(), check(L.zkmi_groth16_verify_each(
                    ctx.h, vk.h, nb, ip, ap, bpp, cp, vp_, ctypes.byref(st)))),
                "decode_loop": decode_loop,
            }
            times = {k: [] for k in calls}
            for rep in range(REPS + 1):  # the first round warms
                for k, fn in calls.items():
                    valid[:] = 0
                    t0 = time.perf_counter()
                    fn()
                    dt = 1e3 * (time.perf_counter() - t0)
                    if k != "decode_loop":
                        assert valid.all() and not mal.any(), k
                    if rep:
                        times[k].append(dt)
            row = {"nb": nb, "fmt": names[fmt], "reps": REPS}
            for k, t in times.items():
                row[k + "_ms"] = round(statistics.median(t), 3)
                row[k + "_spread_ms"] = round(max(t) - min(t), 3)
            row["many_speedup"] = round(row["many_host_decode_ms"] / row["many_encoded_ms"], 3)
            row["each_speedup"] = round(row["each_host_decode_ms"] / row["each_encoded_ms"], 3)
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(3):
                calls["many_encoded"]()
            t, cnt = ctx.profile_get("verify_decode")
            row["verify_decode_ms"] = round(t / max(cnt, 1), 4)
            ctx.profile(False)
            print(json.dumps(row), flush=True)


def main():
    from zelana_amd import gpu
    from zelana_amd.keygen import circuit_specific_setup
    from zelana_amd.r1cs import square_circuit
    from zelana_amd.rng import StdRng
    args = sys.argv[1:]
    each = "--each" in args
    fmts = None
    if "--encoded" in args:
        k = args.index("--encoded")
        name = args[k + 1]
        fmts = sorted(gpu.PROOF_FORMATS.values()) if name == "all" else [gpu.PROOF_FORMATS[name]]
        del args[k:k + 2]
    nbs = [int(a) for a in args if a != "--each"] or [1, 64, 1024]
    ctx = gpu.Context(0)
    cs, _ = square_circuit(2)
    pk, vkb = circuit_specific_setup(ctx, cs, StdRng.seed_from_u64(7))
    vk = gpu.VerifyingKey(ctx, vkb)
    rng = np.random.default_rng(11)
    base, base_in = [], []
    for x in range(2, 66):
        _, z = square_circuit(x)
        zz = np.array([[(v >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in z], np.uint64)
        r, s = (int.from_bytes(rng.bytes(31), "little") for _ in range(2))
        base.append(gpu.groth16_prove(ctx, pk, cs, zz, r, s))
        base_in.append([x * x % R])
    if each:
        each_mode(ctx, vk, vkb, base, base_in, nbs)
        nbs = []
    if fmts is not None:
        encoded_mode(ctx, vk, base, base_in, nbs, fmts)
        nbs = []
    for nb in nbs:
        proofs = [base[i % 64] for i in range(nb)]
        inputs = [base_in[i % 64] for i in range(nb)]
        valid, st = gpu.groth16_verify_many(ctx, vk, proofs, inputs)  # warm
        assert all(valid), "a valid proof was rejected"
        times = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            valid, st = gpu.groth16_verify_many(ctx, vk, proofs, inputs)
            times.append(1e3 * (time.perf_counter() - t0))
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(3):
            gpu.groth16_verify_many(ctx, vk, proofs, inputs)
        prep, nprep = ctx.profile_get("verify_prepare")
        mil, nmil = ctx.profile_get("verify_miller")
        ctx.profile(False)
        call_ms = statistics.median(times)
        nh = min(nb, HOST_CAP)
        t0 = time.perf_counter()
        hv = [gpu.groth16_verify(vkb, inputs[i], *proofs[i]) for i in range(nh)]
        host_ms = 1e3 * (time.perf_counter() - t0) * nb / nh
        assert all(hv)
        bad_in = [list(x) for x in inputs]
        bad_in[nb // 2] = [(bad_in[nb // 2][0] + 1) % R]
        t0 = time.perf_counter()
        bvalid, bst = gpu.groth16_verify_many(ctx, vk, proofs, bad_in)
        bad_ms = 1e3 * (time.perf_counter() - t0)
        assert bvalid == [i != nb // 2 for i in range(nb)]
        print(json.dumps({
            "nb": nb, "reps": REPS, "verify_many_ms": round(call_ms, 3), "verify_many_min_ms": round(min(times), 3),
            "per_proof_ms": round(call_ms / nb, 4), "host_loop_ms": round(host_ms, 3),
            "host_per_proof_ms": round(host_ms / nb, 4), "host_loop_proofs_timed": nh,
            "verify_prepare_ms": round(prep / max(nprep, 1), 3), "verify_miller_ms": round(mil / max(nmil, 1), 3),
            "pairs": st["pairs"], "final_exps": st["final_exps"], "speedup": round(host_ms / call_ms, 2),
            "one_bad_ms": round(bad_ms, 3), "one_bad_final_exps": bst["final_exps"]}), flush=True)
    vk.close()
    pk.close()
    ctx.close()


if __name__ == "__main__":
    main()
