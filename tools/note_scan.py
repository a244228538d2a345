"""Dev tool: measure the encrypted-note store's scan.

    python tools/note_scan.py [--out profiles/note_scan/measure.jsonl] [--reps 5]
                              [--log2 16 18 20] [--keys 1 8] [--hits 8]

Wall time of whole calls (keys in, results on the host out), median and
minimum over --reps after one warm-up call, and the per-kernel split of the
last call from the library's event timers.

A store is filled with 2^e notes of 100-byte ciphertexts.  Notes that are not
addressed to a scanning key are random bytes: they fail the tag exactly as a
foreign note does, and the ladder, the key derivation and the MAC cost the
same whatever the bytes.  --hits real notes for the first key, made by the
model (zelana_amd/note_crypt.py), sit at random indices; the scan must return
exactly those.

For orientation only, per (key, note) pair: the Python model, and, where
ctypes finds OpenSSL 3's libcrypto, a single-thread loop over the same pile
with its X25519 and ChaCha20-Poly1305 (the BLAKE3 compression between them is
left out: libcrypto has none, and it is a few percent of a pair).

One raw JSON line per measurement."""
import argparse
import ctypes
import ctypes.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zelana_amd import gpu, note_crypt as NC  # noqa: E402
from zelana_amd._lib import lib  # noqa: E402

CT_LEN = 100
KERNELS = ["note_scan_ecdh", "note_scan_tag", "note_scan_compact", "note_scan_open", "note_scan_memo"]


def stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "reps": len(ts)}


def profile(ctx):
    out = {}
    for k in KERNELS:
        ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
        if lib().zkmi_profile_get(ctx.h, k.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0 and cnt.value:
            out[k] = ms.value / cnt.value
    return out


def fill(store, rng, n, sk, owner, hits, commit):
    """-> the hit notes, as the scan must return them"""
    where = sorted(rng.choice(n, size=hits, replace=False).tolist())
    pk = NC.public_key(sk)
    want = []
    chunk = 1 << 16
    for first in range(0, n, chunk):
        m = min(chunk, n - first)
        cm = np.frombuffer(rng.bytes(32 * m), np.uint8).reshape(m, 32).copy()
        epk = np.frombuffer(rng.bytes(32 * m), np.uint8).reshape(m, 32).copy()
        nonce = np.frombuffer(rng.bytes(12 * m), np.uint8).reshape(m, 12).copy()
        cts = np.frombuffer(rng.bytes(CT_LEN * m), np.uint8).reshape(m, CT_LEN).copy()
        for i in (w for w in where if first <= w < first + m):
            value, rand, memo = 7 + i, rng.bytes(32), rng.bytes(CT_LEN - 58)
            e, nc, ct = NC.encrypt_note(value, rand, pk, memo, esk=rng.bytes(32), nonce=rng.bytes(12))
            c = commit(owner, value, rand)
            j = i - first
            cm[j], epk[j], nonce[j], cts[j] = (np.frombuffer(x, np.uint8) for x in (c, e, nc, ct))
            want.append((i, c, value, rand, memo))
        store.append_arrays(np.arange(first, first + m, dtype=np.uint32), cm, epk, nonce,
                            np.full(m, CT_LEN, np.uint32), cts)
    return want


def libcrypto_pairs_per_s(notes, sk, seconds=2.0):
    """a single-thread libcrypto loop over (epk, nonce, ct): X25519, then the AEAD open"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_note_crypt_vectors as V
        L = V.load_libcrypto()
    except (SystemExit, OSError, AttributeError):
        return None
    vp, cp, ip = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int
    L.EVP_DecryptInit_ex.argtypes = [vp, vp, vp, cp, cp]
    L.EVP_DecryptUpdate.argtypes = [vp, cp, ctypes.POINTER(ip), cp, ip]
    L.EVP_DecryptFinal_ex.argtypes = [vp, cp, ctypes.POINTER(ip)]
    out, n_, done = ctypes.create_string_buffer(CT_LEN), ip(0), 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for epk, nonce, ct in notes:
            shared, _ = V.ossl_x25519(L, sk, epk)
            c = L.EVP_CIPHER_CTX_new()
            L.EVP_DecryptInit_ex(c, L.EVP_chacha20_poly1305(), None, None, None)
            L.EVP_CIPHER_CTX_ctrl(c, V.CTRL_AEAD_SET_IVLEN, 12, None)
            L.EVP_DecryptInit_ex(c, None, None, shared, nonce)
            L.EVP_DecryptUpdate(c, out, ctypes.byref(n_), ct[:-16], len(ct) - 16)
            L.EVP_CIPHER_CTX_ctrl(c, V.CTRL_AEAD_SET_TAG, 16, ctypes.cast(ctypes.c_char_p(ct[-16:]), vp))
            L.EVP_DecryptFinal_ex(c, out, ctypes.byref(n_))
            L.EVP_CIPHER_CTX_free(c)
            done += 1
    return done / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "note_scan", "measure.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2", type=int, nargs="*", default=[16, 18, 20])
    ap.add_argument("--keys", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--hits", type=int, default=8)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    from zelana_amd.shielded import note_commitment, shielded_hasher
    rng = np.random.default_rng(29)
    ctx = gpu.Context(0)
    poseidon = shielded_hasher(ctx)
    commit = lambda owner, value, rand: note_commitment(value, rand, owner).to_bytes(32, "little")
    sks = [rng.bytes(32) for _ in range(max(a.keys))]
    owners = [rng.bytes(32) for _ in range(max(a.keys))]
    with open(a.out, "a") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(rec, flush=True)

        sample = None
        for e in a.log2:
            n = 1 << e
            store = gpu.NoteStoreDevice(ctx, n, CT_LEN, poseidon=poseidon)
            t0 = time.perf_counter()
            want = fill(store, rng, n, sks[0], owners[0], a.hits, commit)
            emit({"what": "fill", "notes": n, "ct_len": CT_LEN, "s": time.perf_counter() - t0})
            sample = store.get(0, 256)
            for nk in a.keys:
                ts = []
                for rep in range(a.reps + 2):  # a warm-up, the timed calls, one more under the event timers
                    if rep == a.reps + 1:
                        lib().zkmi_profile_reset(ctx.h)
                        lib().zkmi_profile_enable(ctx.h, 1)
                    t0 = time.perf_counter()
                    got = store.scan(sks[:nk], owners[:nk], gpu.COMMIT_POSEIDON)
                    ts.append(time.perf_counter() - t0)
                split = profile(ctx)
                lib().zkmi_profile_enable(ctx.h, 0)
                hits = [(h.position, h.commitment, h.value, h.randomness, h.memo) for h in got[0][0]]
                assert hits == want, "the scan did not return exactly the notes put in"
                assert all(g[0] == [] for g in got[1:])
                emit({"what": "scan", "notes": n, "keys": nk, "pairs": n * nk, "hits": len(hits), **stats(ts[1:-1]),
                      "profiled_call_ms": 1e3 * ts[-1], "kernel_ms": split,
                      "ns_per_pair": 1e9 * statistics.median(ts[1:-1]) / (n * nk)})
            store.close()
        # orientation: the model and libcrypto, one thread, per pair
        pairs = [(x[2], x[3], x[4]) for x in sample]
        t0 = time.perf_counter()
        for epk, nonce, ct in pairs[:64]:
            NC.classify((epk, nonce, ct), sks[0], owners[0], bytes(32))
        emit({"what": "python_model", "us_per_pair": 1e6 * (time.perf_counter() - t0) / 64})
        rate = libcrypto_pairs_per_s(pairs, sks[0])
        emit({"what": "libcrypto_one_thread", "pairs_per_s": rate, "us_per_pair": None if not rate else 1e6 / rate,
              "note": "X25519 + ChaCha20-Poly1305 open through ctypes; no BLAKE3"})
    poseidon.close()
    ctx.close()


if __name__ == "__main__":
    main()
