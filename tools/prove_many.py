"""Dev tool: batched proving (zkmi_groth16_prove_many, Groth16Prover.prove_many)
against the loops a caller has without it.  Prints one JSON line.

    python tools/prove_many.py baseline          # resident loop and two-in-flight submit/wait loop
    python tools/prove_many.py product           # prove_many, nb = 1 .. 64, raw and end to end
    python tools/prove_many.py sweep [lo hi]     # synthetic keys 2^lo .. 2^hi: batched against pipelined
    python tools/prove_many.py groups            # product shape: group size 4 .. 64 at nb = 16 and 64
    python tools/prove_many.py --check [big]     # the R1CS check: off (also on an older library), on, stand-alone

`baseline` uses only entry points older than prove_many, so it also runs on
an older libzkmi.so (ZKMI_LIB=...): build the commit to compare against and
alternate the two in one session.  Product shape: L2BlockCircuit.dummy(), GPU
keygen, fixed-base tables.  Every point is warmed, then timed over a window of
at least PM_WINDOW seconds (default 0.5) that ends in a wait on the results.
"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW = float(os.environ.get("PM_WINDOW", "0.5"))


def timed(fn, per_call):
    """ms per proof of fn() (per_call proofs each) over >= WINDOW s, after two warm calls"""
    fn()
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= WINDOW:
            return round(1e3 * dt / (n * per_call), 4)


def digest(proof):
    return hashlib.sha256(b"".join(np.asarray(x).tobytes() for x in proof)).hexdigest()[:16]


def product_setup():
    from zelana_amd import gpu
    from zelana_amd.keygen import circuit_specific_setup
    from zelana_amd.l2block import L2BlockCircuit
    from zelana_amd.prover import (AccountStateSnapshot, BatchPublicInputs, BatchWitness, Transfer, _as_z,
                                   l2_block_circuit)
    from zelana_amd.rng import StdRng
    ctx = gpu.Context(0)
    cs0, _, _ = L2BlockCircuit.dummy().synthesize()
    pk, vk = circuit_specific_setup(ctx, cs0, StdRng.seed_from_u64(0))
    pk.precompute()
    sender, recipient = bytes([1] * 32), bytes([2] * 32)
    w = BatchWitness(transactions=[Transfer(sender, recipient, 100)],
                     pre_account_states=[AccountStateSnapshot(sender, 1000), AccountStateSnapshot(recipient, 0)])
    inp = BatchPublicInputs(batch_id=42, batch_hash=bytes(range(32)))
    cs, z = l2_block_circuit(inp, w)
    rng = StdRng.seed_from_u64(42)
    r, s = rng.fr_rand(), rng.fr_rand()
    return ctx, pk, vk, gpu.R1CSDevice(ctx, cs), _as_z(z), r, s, (inp, w)


def loops(gpu, ctx, pk, dev, dz, r, s):
    """the two loops available without prove_many: one resident proof at a time, and two in flight"""
    out = {}
    out["resident_ms"] = timed(lambda: gpu.groth16_prove_resident(ctx, pk, dev, dz, r, s), 1)

    def two_in_flight(k=16):
        jobs = [gpu.groth16_prove_submit(ctx, pk, dev, dz, r, s), gpu.groth16_prove_submit(ctx, pk, dev, dz, r, s)]
        last = None
        for i in range(k):
            last = gpu.groth16_prove_wait(jobs.pop(0))
            if i + 2 < k:
                jobs.append(gpu.groth16_prove_submit(ctx, pk, dev, dz, r, s))
        return last

    out["two_in_flight_ms"] = timed(two_in_flight, 16)
    out["proof"] = digest(gpu.groth16_prove_resident(ctx, pk, dev, dz, r, s))
    return out


def leg_baseline():
    from zelana_amd import gpu
    ctx, pk, vk, dev, z, r, s, _ = product_setup()
    dz = gpu.DeviceBuffer(ctx, z.nbytes)
    dz.upload(z)
    return loops(gpu, ctx, pk, dev, dz, r, s)


def leg_product():
    from zelana_amd import gpu
    from zelana_amd.prover import BatchPublicInputs, Groth16Prover
    ctx, pk, vk, dev, z, r, s, (inp, w) = product_setup()
    nbs = [1, 2, 4, 8, 16, 32, 64]
    stride = z.nbytes
    dz = gpu.DeviceBuffer(ctx, max(nbs) * stride)
    dz.upload(np.tile(z.reshape(1, -1), (max(nbs), 1)))
    out = {"group": ctx.batch_group(), "prove_many_ms": {}, "end_to_end_ms": {}, "proofs": {}}
    out.update(loops(gpu, ctx, pk, dev, dz.view(0, stride), r, s))  # the untouched single paths, same build
    for nb in nbs:
        fn = lambda: gpu.groth16_prove_many(ctx, pk, dev, dz, nb, stride, [r] * nb, [s] * nb)
        out["prove_many_ms"][nb] = timed(fn, nb)
        ds = {digest(p) for p in fn()}
        out["proofs"][nb] = ds.pop() if len(ds) == 1 else "MIXED"
    prover = Groth16Prover(ctx, pk, vk)
    prover.prove(inp, w)  # records the shape
    for nb in nbs:
        batches = [(BatchPublicInputs(**{**inp.__dict__, "batch_id": 1000 + i}), w) for i in range(nb)]
        out["end_to_end_ms"][nb] = timed(lambda: prover.prove_many(batches), nb)
    # one hash across every nb, and it is the single resident proof's
    out["identical_across_nb"] = set(out["proofs"].values()) == {out["proof"]}
    return out


def leg_groups():
    from zelana_amd import gpu
    ctx, pk, vk, dev, z, r, s, _ = product_setup()
    stride = z.nbytes
    dz = gpu.DeviceBuffer(ctx, 64 * stride)
    dz.upload(np.tile(z.reshape(1, -1), (64, 1)))
    out = {}
    for nb in (16, 64):
        for group in (4, 8, 16, 32, 64):
            ctx.set_batch_group(group)
            out[f"nb{nb}_g{group}_ms"] = timed(
                lambda: gpu.groth16_prove_many(ctx, pk, dev, dz, nb, stride, [r] * nb, [s] * nb), nb)
    ctx.set_batch_group(0)
    return out


def leg_sweep(lo, hi):
    from zelana_amd import gpu
    from zelana_amd.r1cs import synthetic_fast
    ctx = gpu.Context(0)
    out = {}
    for log_n in range(lo, hi + 1):
        m = (1 << log_n) - 8
        cs, z = synthetic_fast(m, 4, m, seed=log_n)
        pk = gpu.synthetic_pk(ctx, 70 + log_n, log_n, 4, m)
        pk.precompute()
        dev = gpu.R1CSDevice(ctx, cs)
        stride = z.nbytes
        dz = gpu.DeviceBuffer(ctx, 16 * stride)
        dz.upload(np.tile(z.reshape(1, -1), (16, 1)))
        row = loops(gpu, ctx, pk, dev, dz.view(0, stride), 3, 4)
        for nb, group in ((1, 0), (4, 0), (16, 0), (16, 2), (16, 4), (16, 8), (16, 16)):
            ctx.set_batch_group(group)
            fn = lambda: gpu.groth16_prove_many(ctx, pk, dev, dz, nb, stride, [3] * nb, [4] * nb)
            row[f"many_nb{nb}_g{group}_ms"] = timed(fn, nb)
            row[f"same_nb{nb}_g{group}"] = all(digest(p) == row["proof"] for p in fn())
        ctx.set_batch_group(0)
        out[log_n] = row
        dz.free()
        dev.close()
        pk.close()
    return out


def leg_check(big):
    """Product shape: the single resident proof and prove_many at nb = 1 and 64
    with the prove check off (these entry points exist in an older libzkmi.so
    too: ZKMI_LIB=...), then on, and the stand-alone zkmi_r1cs_check.  big: also
    one large proof (2^17 synthetic key) off and on, and the stand-alone check
    of the 2^21 zelana_batch shape (batch 70) beside the download of its z."""
    from zelana_amd import gpu
    from zelana_amd._lib import lib
    ctx, pk, vk, dev, z, r, s, _ = product_setup()
    stride = z.nbytes
    dz = gpu.DeviceBuffer(ctx, 64 * stride)
    dz.upload(np.tile(z.reshape(1, -1), (64, 1)))
    has = hasattr(lib(), "zkmi_r1cs_check")

    def point(fn1, fnm):
        row = {"resident_ms": timed(fn1, 1)}
        for nb in (1, 64):
            row[f"many_nb{nb}_ms"] = timed(lambda: fnm(nb), nb)
        row["proofs"] = sorted({digest(fn1())} | {digest(p) for nb in (1, 64) for p in fnm(nb)})
        return row

    fn1 = lambda: gpu.groth16_prove_resident(ctx, pk, dev, dz.view(0, stride), r, s)
    fnm = lambda nb: gpu.groth16_prove_many(ctx, pk, dev, dz, nb, stride, [r] * nb, [s] * nb)
    out = {"has_check": has, "off": point(fn1, fnm)}
    if has:
        ctx.set_prove_check(True)
        out["on"] = point(fn1, fnm)
        st = gpu.groth16_last_check(ctx)
        out["on"]["statuses"] = len(st)
        out["on"]["first_row"], out["on"]["n_bad"] = st[0].first_row, st[0].n_bad
        ctx.set_prove_check(False)
        out["same_proofs"] = out["on"]["proofs"] == out["off"]["proofs"]
        for nb in (1, 64):
            out[f"standalone_nb{nb}_ms"] = timed(lambda: gpu.r1cs_check(ctx, dev, dz, nb, stride), nb)
    if big:
        from zelana_amd.r1cs import synthetic_fast
        m = (1 << 17) - 8
        cs2, z2 = synthetic_fast(m, 4, m, seed=17)
        pk2 = gpu.synthetic_pk(ctx, 87, 17, 4, m)
        pk2.precompute()
        dev2 = gpu.R1CSDevice(ctx, cs2)
        dz2 = gpu.DeviceBuffer(ctx, z2.nbytes)
        dz2.upload(z2)
        big1 = lambda: gpu.groth16_prove_resident(ctx, pk2, dev2, dz2, 3, 4)
        out["big17_off_ms"] = timed(big1, 1)
        if has:
            ctx.set_prove_check(True)
            out["big17_on_ms"] = timed(big1, 1)
            ctx.set_prove_check(False)
            out["big17_standalone_ms"] = timed(lambda: gpu.r1cs_check(ctx, dev2, dz2), 1)
        for o in (dz2, dev2, pk2):
            (o.free if hasattr(o, "free") else o.close)()
        if has:
            from zelana_amd import zbatch
            d = zbatch.load_prover_toml(os.path.join(ROOT, "tests", "golden", "zelana_batch_70_Prover.toml"))
            cs3, z3, _ = zbatch.build(d)
            dev3 = gpu.R1CSDevice(ctx, cs3)
            dz3 = gpu.DeviceBuffer(ctx, z3.nbytes)
            dz3.upload(z3)
            st3 = gpu.r1cs_check(ctx, dev3, dz3)[0]
            out["batch70"] = {"m": cs3.num_constraints, "z_mb": round(z3.nbytes / 2**20, 1),
                              "first_row": st3.first_row, "n_bad": st3.n_bad,
                              "standalone_ms": timed(lambda: gpu.r1cs_check(ctx, dev3, dz3), 1),
                              "download_z_ms": timed(lambda: dz3.download(np.empty_like(z3)), 1)}
    return out


def main():
    leg = sys.argv[1] if len(sys.argv) > 1 else "product"
    if leg == "baseline":
        res = leg_baseline()
    elif leg == "product":
        res = leg_product()
    elif leg == "groups":
        res = leg_groups()
    elif leg in ("check", "--check"):
        res = leg_check(len(sys.argv) > 2 and sys.argv[2] == "big")
    elif leg == "sweep":
        res = leg_sweep(int(sys.argv[2]) if len(sys.argv) > 2 else 10, int(sys.argv[3]) if len(sys.argv) > 3 else 18)
    else:
        raise SystemExit(__doc__)
    from zelana_amd._lib import LIB_PATH
    print(json.dumps({"leg": leg, "lib": os.path.relpath(LIB_PATH, ROOT), "window_s": WINDOW, **res}), flush=True)


if __name__ == "__main__":
    main()
