"""Dev tool: ShieldedTransferCircuit at its real shape (2 inputs, 2 outputs,
depth-32 paths: 18,927 constraints, 2^15 domain) through ShieldedProver,
against what a caller has without it.  Prints one JSON line per point.

    python tools/shielded.py [nb ...]        # default 1 64 256

Per nb, every figure is the median of REPS (11) calls after a warm call, the
raw times kept in the line ("raw"):
  inputs_ms       witness_inputs() of nb transfers (host)
  wprog_ms        run_many of the witness program, kernel time (the library's
                  "wprog" timer) -- as scheduled (runs of small levels in one
                  k_wprog_chain launch) and with one launch per level
                  (wprog_per_level_ms; ZKMI_DEBUG_WPROG_NO_RC_CHAIN=1), alternated
  prove_many_ms   ShieldedProver.prove_many end to end, per proof
  r1cs_check_ms   gpu.r1cs_check of the nb resident assignments
  verify_many_ms, verify_each_ms   over the nb proofs, per proof
  baseline_ms     one proof without the witness program: Python synthesize(),
                  upload of z, groth16_prove_resident -- one call of it before
                  every prove_many call, so the two alternate in one session
The transfers are 4 distinct honest ones repeated (making 256 in Python would
take minutes of hashing); every proof has its own r, s.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("SH_REPS", "11"))


def honest(salt):
    from zelana_amd import shielded as S
    tree = S.NoteTree(32)
    tree.insert(0, 12345)
    ins = tree.spend_notes([(100 + salt, bytes([10 + salt] * 32), bytes([20 + salt] * 32), 1),
                            (50 + salt, bytes([11 + salt] * 32), bytes([21 + salt] * 32), (1 << 32) - 2)])
    outs = [S.OutputNote(140 + 2 * salt, bytes([30] * 32), bytes([40] * 32)),
            S.OutputNote(7, bytes([31] * 32), bytes([41] * 32))]
    return S.ShieldedTransfer.honest(ins, outs)


def med(xs):
    return round(statistics.median(xs), 4)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    from zelana_amd import gpu, shielded as S, wprog as W
    from zelana_amd._lib import LIB_PATH
    nbs = [int(a) for a in sys.argv[1:]] or [1, 64, 256]
    ctx = gpu.Context(0)
    t0 = time.perf_counter()
    sp = S.ShieldedProver(ctx, (32, 32, 2), seed=0)
    setup_s = round(time.perf_counter() - t0, 2)
    os.environ["ZKMI_DEBUG_WPROG_NO_RC_CHAIN"] = "1"
    wp_levels = W.WitnessProgram(ctx, sp.program)
    del os.environ["ZKMI_DEBUG_WPROG_NO_RC_CHAIN"]
    base = [honest(s) for s in range(4)]
    head = {"lib": os.path.relpath(LIB_PATH, ROOT), "shape": [32, 32, 2], "constraints": sp.r1cs.num_constraints,
            "domain": sp.pk.n, "vars": sp.program.num_vars, "levels": sp.program.num_levels,
            "ops": int(sp.program.op.shape[0]), "reps": REPS, "setup_s": setup_s}

    def baseline(t, seed):
        from zelana_amd.rng import StdRng
        cs, z, _ = S.synthesize(t)
        dz = sp.z_buffer(1)
        dz.upload(S.z_limbs(z))
        rng = StdRng.seed_from_u64(seed)
        return gpu.groth16_prove_resident(ctx, sp.pk, sp.dev, dz, rng.fr_rand(), rng.fr_rand())

    def wprog_ms(wp, inputs, dz, nb):
        ctx.profile(True)
        ctx.profile_reset()
        wp.run_many(inputs, dz, sp.stride)
        t, _ = ctx.profile_get("wprog")
        ctx.profile(False)
        return t

    for nb in nbs:
        ts = [base[i % 4] for i in range(nb)]
        seeds = list(range(1000, 1000 + nb))
        inputs = [S.witness_inputs(t) for t in ts]
        dz = sp.z_buffer(nb)
        raw = {k: [] for k in ("inputs_ms", "wprog_ms", "wprog_per_level_ms", "prove_many_ms", "r1cs_check_ms",
                               "verify_many_ms", "verify_each_ms", "baseline_ms")}
        proofs = None
        for rep in range(REPS + 1):
            row = {}
            row["inputs_ms"] = ms(lambda: [S.witness_inputs(t) for t in ts])
            row["wprog_ms"] = wprog_ms(sp.wp, inputs, dz, nb)
            row["wprog_per_level_ms"] = wprog_ms(wp_levels, inputs, dz, nb)
            row["r1cs_check_ms"] = ms(lambda: gpu.r1cs_check(ctx, sp.dev, dz, nb, sp.stride))
            row["baseline_ms"] = ms(lambda: baseline(ts[rep % nb], seeds[rep % nb]))
            t0 = time.perf_counter()
            proofs = sp.prove_many(ts, seeds)
            row["prove_many_ms"] = (time.perf_counter() - t0) * 1e3 / nb
            row["verify_many_ms"] = ms(lambda: sp.verify_many(proofs)) / nb
            row["verify_each_ms"] = ms(lambda: sp.verify_each(proofs)) / nb
            if rep:  # rep 0 warms
                for k, v in row.items():
                    raw[k].append(round(v, 4))
        ok = sp.verify_each(proofs)
        one = baseline(ts[0], seeds[0])
        st = gpu.r1cs_check(ctx, sp.dev, sp.z_buffer(nb), 1, sp.stride)[0]
        print(json.dumps({**head, "nb": nb, **{k: med(v) for k, v in raw.items()}, "all_valid": all(ok),
                          "same_proof_as_baseline": all(np.array_equal(x, y) for x, y in
                                                        zip(one, (proofs[0].a, proofs[0].b, proofs[0].c))),
                          "satisfied": st.first_row is None, "raw": raw}), flush=True)
    wp_levels.close()
    sp.close()


if __name__ == "__main__":
    main()
