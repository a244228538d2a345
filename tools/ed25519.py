"""Dev tool: measure batched Ed25519 verification.

    python tools/ed25519.py [--out profiles/ed25519/measure.jsonl] [--reps 5]
                            [--log2 10 16 20] [--distinct 4096]

Wall time of whole zkmi_ed25519_verify_many calls over ready arrays (keys,
signatures and messages in, verdicts on the host out), median and minimum over
--reps after one warm-up call, and the per-kernel split of one further call
from the library's event timers.

The pile: --distinct honest signatures over transfer-format messages
(ed25519.transfer_message, about 235 bytes: three SHA-512 blocks with R and A),
signed by libcrypto where ctypes finds it and by the Python model otherwise,
repeated up to 2^e.  Neither kernel's work depends on the bytes, so a repeated
signature costs what a fresh one does.  Each size runs twice: all honest, and
with 1 % of the signatures spoiled (a bit of s, of R, or a key on no point, in
turn) at random places; the verdicts are checked against what was put in.

For orientation only: a single-thread loop over libcrypto's EVP_DigestVerify
on this host, the Python model, and tx_auth.verify_transfers end to end over
SignedTransfer objects, where the Python message formatting is timed apart
from the device call.

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

KERNELS = ["ed25519_hash", "ed25519_curve"]


def stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "reps": len(ts)}


def profile(ctx):
    out = {}
    for k in KERNELS:
        ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
        if lib().zkmi_profile_get(ctx.h, k.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0 and cnt.value:
            out[k] = ms.value / cnt.value
    return out


def libcrypto():
    try:
        import make_ed25519_vectors as V
        return V, V.load_libcrypto()
    except (SystemExit, OSError, AttributeError):
        return None, None


def make_pile(rng, distinct):
    """-> (pks, sigs, msgs, signer): `distinct` honest transfer-format triples"""
    V, C = libcrypto()
    seeds = [rng.bytes(32) for _ in range(64)]
    pks = [E.public_key(s) for s in seeds]
    out_pk, out_sig, out_msg = [], [], []
    for i in range(distinct):
        j = i % len(seeds)
        msg = E.transfer_message(pks[j], pks[(j + 1) % len(seeds)], int(rng.integers(1, 2**40)), i, 1)
        sig = V.ossl_keypair_sign(C, seeds[j], msg)[1] if C is not None else E.sign(seeds[j], msg)
        out_pk.append(pks[j]), out_sig.append(sig), out_msg.append(msg)
    return out_pk, out_sig, out_msg, "libcrypto" if C is not None else "python model"


def tile(pks, sigs, msgs, n):
    """the pile repeated to n signatures, as the arrays verify_arrays takes"""
    d = len(pks)
    reps = (n + d - 1) // d
    pk = np.tile(np.frombuffer(b"".join(pks), np.uint8).reshape(d, 32), (reps, 1))[:n].copy()
    sg = np.tile(np.frombuffer(b"".join(sigs), np.uint8).reshape(d, 64), (reps, 1))[:n].copy()
    lens = np.tile(np.array([len(m) for m in msgs], np.uint64), reps)[:n]
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    blob = np.frombuffer(b"".join(msgs), np.uint8)
    ms = np.concatenate([np.tile(blob, n // d), np.frombuffer(b"".join(msgs[:n % d]) or b"", np.uint8)])
    assert ms.size == int(off[-1])
    return pk, sg, ms, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ed25519", "measure.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2", type=int, nargs="*", default=[10, 16, 20])
    ap.add_argument("--distinct", type=int, default=4096)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rng = np.random.default_rng(31)
    ctx = gpu.Context(0)
    ver = gpu.Ed25519Verifier(ctx)
    with open(a.out, "a") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(rec, flush=True)

        t0 = time.perf_counter()
        pks, sigs, msgs, signer = make_pile(rng, a.distinct)
        emit({"what": "pile", "distinct": a.distinct, "signer": signer, "s": time.perf_counter() - t0,
              "msg_bytes_mean": sum(map(len, msgs)) / len(msgs)})
        best_ns = None
        for e in a.log2:
            n = 1 << e
            pk, sg, ms, off = tile(pks, sigs, msgs, n)
            for bad_share in (0.0, 0.01):
                want = np.zeros(n, np.uint8)
                pk2, sg2 = pk, sg
                if bad_share:
                    pk2, sg2 = pk.copy(), sg.copy()
                    where = rng.choice(n, size=max(1, int(n * bad_share)), replace=False)
                    for j, i in enumerate(where.tolist()):
                        if j % 3 == 0:
                            sg2[i, 32] ^= 1
                            want[i] = E.SIG_MISMATCH
                        elif j % 3 == 1:
                            sg2[i, 1] ^= 4
                            want[i] = E.SIG_MISMATCH
                        else:
                            pk2[i] = np.frombuffer((2).to_bytes(32, "little"), np.uint8)
                            want[i] = E.SIG_BAD_PUBKEY
                ts = []
                for rep in range(a.reps + 2):  # a warm-up, the timed calls, one more under the event timers
                    if rep == a.reps + 1:
                        lib().zkmi_profile_reset(ctx.h)
                        lib().zkmi_profile_enable(ctx.h, 1)
                    t0 = time.perf_counter()
                    got = ver.verify_arrays(pk2, sg2, ms, off)
                    ts.append(time.perf_counter() - t0)
                split = profile(ctx)
                lib().zkmi_profile_enable(ctx.h, 0)
                assert np.array_equal(got, want), "the verdicts are not what was put in"
                ns = 1e9 * statistics.median(ts[1:-1]) / n
                if not bad_share:
                    best_ns = ns if best_ns is None else min(best_ns, ns)
                emit({"what": "verify_many", "n": n, "bad_share": bad_share, "bad": int((want != 0).sum()),
                      **stats(ts[1:-1]), "profiled_call_ms": 1e3 * ts[-1], "kernel_ms": split, "ns_per_signature": ns,
                      "curve_ns_per_signature": None if "ed25519_curve" not in split else 1e6 * split["ed25519_curve"] / n})

        # orientation: libcrypto, one thread, and the model
        V, C = libcrypto()
        lc_us = None
        if C is not None:
            done, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < 2.0:
                for p, m, s in zip(pks[:256], msgs[:256], sigs[:256]):
                    assert V.ossl_verify(C, p, m, s)
                    done += 1
            lc_us = 1e6 * (time.perf_counter() - t0) / done
        emit({"what": "libcrypto_one_thread", "us_per_signature": lc_us,
              "note": "EVP_DigestVerify through ctypes, a fresh EVP_PKEY and EVP_MD_CTX per signature"})
        t0 = time.perf_counter()
        for p, m, s in zip(pks[:16], msgs[:16], sigs[:16]):
            assert E.verify(p, m, s) == E.SIG_OK
        model_us = 1e6 * (time.perf_counter() - t0) / 16
        emit({"what": "python_model", "us_per_signature": model_us})

        # verify_transfers end to end: objects in, reasons out; the message formatting timed apart
        nt = min(a.distinct, 4096)
        txs = []
        for p, m, s in zip(pks[:nt], msgs[:nt], sigs[:nt]):
            lines = m.decode().split("\n")
            to, amount, nonce = bytes.fromhex(lines[3][4:]), int(lines[4].split()[1]), int(lines[5].split()[1])
            txs.append(T.SignedTransfer(p, to, amount, nonce, 1, s, p))
        te, tf = [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            reasons, formats = T.verify_transfers(ver, txs)
            te.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for t in txs:
                t.messages()
            tf.append(time.perf_counter() - t0)
        assert reasons == [T.OK] * nt and formats == [T.READABLE] * nt
        emit({"what": "verify_transfers", "n": nt, **stats(te[1:]), "formatting_ms": 1e3 * statistics.median(tf[1:]),
              "formatting_share": statistics.median(tf[1:]) / statistics.median(te[1:]),
              "note": "formatting_ms: both message formats of every transfer built in Python, as verify_transfers builds them"})

        # the two yardsticks: libcrypto on this host, and note_scan's ladder (one X25519 a pair)
        ladder = None
        try:
            with open(os.path.join(ROOT, "profiles", "note_scan", "measure.jsonl")) as g:
                scans = [json.loads(ln) for ln in g if '"scan"' in ln]
            ladder = min(s["ns_per_pair"] for s in scans)
        except (OSError, ValueError, KeyError):
            pass
        emit({"what": "ratios", "ns_per_signature": best_ns, "libcrypto_us": lc_us,
              "libcrypto_over_gpu": None if not lc_us else 1e3 * lc_us / best_ns, "ladder_ns_per_pair": ladder,
              "signature_over_ladder": None if not ladder else best_ns / ladder})
    ctx.close()


if __name__ == "__main__":
    main()
