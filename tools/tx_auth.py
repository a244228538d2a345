"""Dev tool: measure the authorisation of transfers from their fields, the
messages built on the device.

    python tools/tx_auth.py [--out profiles/tx_auth/measure.jsonl] [--reps 5]
                            [--log2 10 12 16 20] [--distinct 4096]

The pile: --distinct honest SignedTransfers, signed by libcrypto where ctypes
finds it and by the Python model otherwise, one in four over the legacy
message, repeated up to 2^e.  No kernel's work depends on the bytes, so a
repeated record costs what a fresh one does.  Per size, wall time as median
and minimum over --reps after one warm-up call:

  pack            tx_auth.pack alone: objects -> records
  auth_records    zkmi_tx_auth_many over ready records, reasons and formats on
                  the host, and the per-kernel split of one further call from
                  the library's event timers
  verify_arrays   the yardstick of the device call: zkmi_ed25519_verify_many
                  over the Python-built messages of the same records, the
                  format each was signed over, in ONE call (it does no retry,
                  so it does less than auth_records: one curve pass, not 1.25)
  verify_transfers  end to end over the objects, with device_messages=True and
                  with False, which is the path from before the device built
                  the messages (sizes up to 2^16: the host path takes seconds
                  beyond)

Every run's reasons and formats are checked against what was put in.  The
2^20 run is the only one that crosses the curve kernel's chunk of 2^18.

One raw JSON line per measurement."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from zelana_amd import ed25519 as E, gpu, tx_auth as T  # noqa: E402
from zelana_amd._lib import lib  # noqa: E402

KERNELS = ["txauth_format", "txauth_hash", "txauth_curve", "txauth_compact", "txauth_format_legacy", "txauth_hash_legacy",
           "txauth_curve_legacy", "txauth_epilogue"]
HOST_PATH_MAX_LOG2 = 16


def stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "reps": len(ts)}


def timed(fn, reps):
    """one warm-up call, then reps timed ones -> (times, last result)"""
    ts, out = [], None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts[1:], out


def profile(ctx, names):
    out = {}
    for k in names:
        ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
        if lib().zkmi_profile_get(ctx.h, k.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0 and cnt.value:
            out[k] = ms.value / cnt.value
    return out


def profiled(ctx, fn, names):
    lib().zkmi_profile_reset(ctx.h)
    lib().zkmi_profile_enable(ctx.h, 1)
    try:
        fn()
        return profile(ctx, names)
    finally:
        lib().zkmi_profile_enable(ctx.h, 0)


def libcrypto():
    try:
        import make_ed25519_vectors as V
        return V, V.load_libcrypto()
    except (SystemExit, OSError, AttributeError):
        return None, None


def make_pile(rng, distinct):
    """-> (transfers, signer): `distinct` honest SignedTransfers, every fourth signed over the legacy message"""
    V, C = libcrypto()
    seeds = [rng.bytes(32) for _ in range(64)]
    pks = [E.public_key(s) for s in seeds]
    txs = []
    for i in range(distinct):
        j = i % len(seeds)
        t = T.SignedTransfer(pks[j], pks[(j + 1) % len(seeds)], int(rng.integers(1, 2**40)), i, 1, b"", pks[j])
        msg = t.messages()[1 if i % 4 == 3 else 0]
        t.signature = V.ossl_keypair_sign(C, seeds[j], msg)[1] if C is not None else E.sign(seeds[j], msg)
        txs.append(t)
    return txs, "libcrypto" if C is not None else "python model"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx_auth", "measure.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2", type=int, nargs="*", default=[10, 12, 16, 20])
    ap.add_argument("--distinct", type=int, default=4096)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rng = np.random.default_rng(37)
    ctx = gpu.Context(0)
    ver = gpu.Ed25519Verifier(ctx)
    with open(a.out, "a") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(rec, flush=True)

        t0 = time.perf_counter()
        pile, signer = make_pile(rng, a.distinct)
        d = len(pile)
        emit({"what": "pile", "distinct": d, "signer": signer, "legacy_share": sum(i % 4 == 3 for i in range(d)) / d,
              "s": time.perf_counter() - t0})
        pile_rec = T.pack(pile)
        pile_msgs = [t.messages()[1 if i % 4 == 3 else 0] for i, t in enumerate(pile)]
        for e in a.log2:
            n = 1 << e
            reps_of_pile = (n + d - 1) // d
            txs = (pile * reps_of_pile)[:n]
            want_r = np.zeros(n, np.uint8)
            want_f = np.tile(np.where(np.arange(d) % 4 == 3, gpu.TXFMT_LEGACY, gpu.TXFMT_READABLE).astype(np.uint8), reps_of_pile)[:n]
            want = ([T.OK] * n, [T.LEGACY if v == gpu.TXFMT_LEGACY else T.READABLE for v in want_f.tolist()])

            ts, rec = timed(lambda: T.pack(txs), a.reps)
            assert rec.tobytes() == np.tile(pile_rec, reps_of_pile)[:n].tobytes()
            emit({"what": "pack", "n": n, **stats(ts), "ns_per_record": 1e9 * statistics.median(ts) / n})

            ts, (r, fm) = timed(lambda: ver.auth_records(rec), a.reps)
            assert np.array_equal(r, want_r) and np.array_equal(fm, want_f), "reasons or formats are not what was put in"
            split = profiled(ctx, lambda: ver.auth_records(rec), KERNELS)
            auth_ms = 1e3 * statistics.median(ts)
            emit({"what": "auth_records", "n": n, **stats(ts), "kernel_ms": split, "ns_per_record": 1e6 * auth_ms / n,
                  "retried": int((want_f == gpu.TXFMT_LEGACY).sum())})

            # the yardstick: verify_arrays over the Python-built messages of the same records
            pk = np.ascontiguousarray(rec["signer_pubkey"])
            sg = np.ascontiguousarray(rec["signature"])
            lens = np.tile(np.array([len(m) for m in pile_msgs], np.uint64), reps_of_pile)[:n]
            off = np.zeros(n + 1, np.uint64)
            np.cumsum(lens, out=off[1:])
            ms = np.frombuffer(b"".join(pile_msgs) * (n // d) + b"".join(pile_msgs[:n % d]), np.uint8)
            ts, v = timed(lambda: ver.verify_arrays(pk, sg, ms, off), a.reps)
            assert not v.any(), "verify_arrays refuses an honest signature"
            split_v = profiled(ctx, lambda: ver.verify_arrays(pk, sg, ms, off), ["ed25519_hash", "ed25519_curve"])
            arrays_ms = 1e3 * statistics.median(ts)
            emit({"what": "verify_arrays", "n": n, **stats(ts), "kernel_ms": split_v, "ns_per_signature": 1e6 * arrays_ms / n,
                  "note": "one call over ready Python-built messages, each in the format it was signed over: no retry"})
            emit({"what": "ratio_device_call", "n": n, "auth_records_over_verify_arrays": auth_ms / arrays_ms})

            if e <= HOST_PATH_MAX_LOG2:
                ts_d, got = timed(lambda: T.verify_transfers(ver, txs, device_messages=True), a.reps)
                assert got == want
                ts_h, got = timed(lambda: T.verify_transfers(ver, txs, device_messages=False), a.reps)
                assert got == want
                emit({"what": "verify_transfers", "n": n, "device_messages": True, **stats(ts_d)})
                emit({"what": "verify_transfers", "n": n, "device_messages": False, **stats(ts_h)})
                emit({"what": "ratio_end_to_end", "n": n,
                      "host_messages_over_device_messages": statistics.median(ts_h) / statistics.median(ts_d)})
    ctx.close()


if __name__ == "__main__":
    main()
