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


def main():
    from zelana_amd import gpu
    from zelana_amd.keygen import circuit_specific_setup
    from zelana_amd.r1cs import square_circuit
    from zelana_amd.rng import StdRng
    nbs = [int(a) for a in sys.argv[1:]] or [1, 64, 1024]
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
