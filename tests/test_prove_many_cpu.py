"""CPU: the batched-proving boundary without a GPU.  include/zkmi.h declares
the batched entry points and libzkmi.so exports them; Groth16Prover.prove_many's
host logic -- grouping by circuit shape, one recording prove() per new shape,
r / s from StdRng::seed_from_u64(batch_id) per item, results in input order,
the item-by-item fallback for a custom synthesizer -- runs against stubs of
the GPU calls."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["zkmi_msm_batch_submit", "zkmi_msm_batch_wait", "zkmi_ntt_batch_device", "zkmi_groth16_prove_many_submit",
       "zkmi_groth16_prove_many_wait", "zkmi_groth16_prove_many", "zkmi_ctx_set_batch_group",
       "zkmi_ctx_get_batch_group"]


def test_header_declares_and_library_exports_batched_entry_points():
    from zelana_amd._lib import LIB_PATH, SIGNATURES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zkmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(zkmi_[a-z0-9_]+)\s*\(", src))
    bound = {n for n, _, _ in SIGNATURES}
    if not os.path.exists(LIB_PATH):
        from zelana_amd.build_native import build
        build()
    L = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in bound, name
        assert hasattr(L, name), name


def test_batch_calls_reject_bad_arguments_without_a_gpu():
    """argument checks that run before any device work"""
    from zelana_amd._lib import lib
    L = lib()
    assert L.zkmi_msm_batch_wait(None, None, 0) == -1
    assert L.zkmi_groth16_prove_many_wait(None, 0, None, None, None) == -1
    assert L.zkmi_ctx_set_batch_group(None, 1) == -1
    assert L.zkmi_ctx_get_batch_group(None) == -1


def _limbs(x):
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


class _Plan:
    num_vars = 6
    template_inputs = np.zeros((2, 4), np.uint64)


class _Buf:
    def __init__(self, ctx, nbytes):
        self.nbytes, self.slots = nbytes, {}


class _WP:
    log = []

    def __init__(self, ctx, plan):
        self.plan = plan

    def run(self, ins, dz, async_=False):
        _WP.log.append(("run", 1))
        dz.slots[0] = np.asarray(ins)

    def run_many(self, ins, dz, stride, async_=False):
        assert stride == _Plan.num_vars * 32 and dz.nbytes >= len(ins) * stride
        _WP.log.append(("run_many", len(ins)))
        for i, x in enumerate(ins):
            dz.slots[i] = np.asarray(x)


def _fake_proof(z_inputs, r, s):
    """points that carry what the call was given: r, s and the witness inputs' batch id"""
    a = np.array(_limbs(r) + _limbs(s), np.uint64)
    b = np.zeros(16, np.uint64)
    b[0] = z_inputs[1, 0]
    c = np.array(_limbs(r ^ s) + [1, 2, 3, 4], np.uint64)
    return a, b, c


def _stub(monkeypatch):
    from zelana_amd import gpu, host_prover as H, wprog
    calls = {"resident": 0, "many": []}
    _WP.log = []
    monkeypatch.setattr(H, "l2_shape_key", lambda inp, wit: wit["shape"])

    def ins_of(inp, wit):
        v = np.zeros((2, 4), np.uint64)
        v[0, 0], v[1, 0] = 1, inp.batch_id
        return v

    monkeypatch.setattr(H, "l2_witness_inputs", ins_of)
    # (the recording prove() of a new shape proves the plan's template inputs: the item's own)
    monkeypatch.setattr(H, "l2_record", lambda inp, wit: (None, None, _plan_for(ins_of(inp, wit))))
    monkeypatch.setattr(wprog, "WitnessProgram", _WP)
    monkeypatch.setattr(gpu, "R1CSDevice", lambda ctx, cs: object())
    monkeypatch.setattr(gpu, "DeviceBuffer", _Buf)

    def resident(ctx, pk, dev, dz, r, s):
        calls["resident"] += 1
        return _fake_proof(dz.slots[0], r, s)

    def many(ctx, pk, dev, dz, nb, stride, rs, ss):
        calls["many"].append(nb)
        return [_fake_proof(dz.slots[i], rs[i], ss[i]) for i in range(nb)]

    monkeypatch.setattr(gpu, "groth16_prove_resident", resident)
    monkeypatch.setattr(gpu, "groth16_prove_many", many)
    return calls, ins_of


def test_prove_many_groups_by_shape_in_input_order(monkeypatch):
    from zelana_amd.host_prover import native_l2_block_circuit
    from zelana_amd.prover import BatchPublicInputs, Groth16Prover
    from zelana_amd.rng import StdRng
    calls, ins_of = _stub(monkeypatch)
    p = Groth16Prover(object(), object(), b"vk", circuit=native_l2_block_circuit)
    ids = [7, 3, 9, 3, 11, 70, 5]
    shapes = ["A", "B", "A", "A", "B", "A", "C"]
    batches = [(BatchPublicInputs(batch_id=i), {"shape": s}) for i, s in zip(ids, shapes)]
    out = p.prove_many(batches)
    assert [o.public_inputs.batch_id for o in out] == ids            # input order
    for o, bid in zip(out, ids):
        rng = StdRng.seed_from_u64(bid)
        r, s = rng.fr_rand(), rng.fr_rand()
        assert list(o.a) == _limbs(r) + _limbs(s)                     # r, s of this item's batch_id
        assert int(o.b[0]) == bid                                     # proved over this item's witness
        assert len(o.proof_bytes) == 256
    # one ordinary prove per new shape (A, B, C), the rest of each group in one batched call
    assert calls["resident"] == 3 and sorted(calls["many"]) == [1, 3]
    assert _WP.log.count(("run", 1)) == 3 and ("run_many", 3) in _WP.log and ("run_many", 1) in _WP.log
    # a second call knows every shape: no recording prove, one batched call per shape
    calls["resident"], calls["many"] = 0, []
    out2 = p.prove_many(batches)
    assert calls["resident"] == 0 and sorted(calls["many"]) == [1, 2, 4]
    assert [o.proof_bytes for o in out2] == [o.proof_bytes for o in out]
    assert p.prove_many([]) == []


def _plan_for(ins):
    pl = _Plan()
    pl.template_inputs = ins
    return pl


def test_prove_many_custom_synthesizer_falls_back_to_a_loop(monkeypatch):
    from zelana_amd import gpu
    from zelana_amd.prover import BatchPublicInputs, Groth16Prover
    from zelana_amd.rng import StdRng
    calls, _ = _stub(monkeypatch)
    seen = []

    def prove(ctx, pk, cs, z, r, s):
        seen.append((cs, r, s))
        return _fake_proof(np.array([[1, 0, 0, 0], [cs, 0, 0, 0]], np.uint64), r, s)

    monkeypatch.setattr(gpu, "groth16_prove", prove)
    p = Groth16Prover(object(), object(), b"vk", circuit=lambda inp, wit: (inp.batch_id, np.zeros((2, 4), np.uint64)))
    ids = [4, 2, 4]
    out = p.prove_many([(BatchPublicInputs(batch_id=i), None) for i in ids])
    assert [o.public_inputs.batch_id for o in out] == ids and [c for c, _, _ in seen] == ids
    for (_, r, s), bid in zip(seen, ids):
        rng = StdRng.seed_from_u64(bid)
        assert (r, s) == (rng.fr_rand(), rng.fr_rand())
    assert calls["many"] == [] and calls["resident"] == 0
