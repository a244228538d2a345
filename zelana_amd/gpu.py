"""Thin Python handle over libzkmi.so for device-resident MSM / NTT / Groth16.

Arrays cross as numpy uint64 (canonical little-endian limbs), matching the C
ABI.  One Context per GPU (one process per GPU, see bench.py).
"""
from __future__ import annotations

import ctypes
import weakref
from dataclasses import dataclass

import numpy as np

from ._lib import (ROW_NONE, R1CSStatusStruct, R1CSStruct, VerifyStatsStruct, ZkmiError, check, lib, u32p, u64p, u8p,
                   vp)


def _p64(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags.c_contiguous
    return a.ctypes.data_as(u64p)


class DeviceBuffer:
    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = vp()
        check(lib().zkmi_dev_alloc(ctx.h, nbytes, ctypes.byref(self.ptr)), "zkmi_dev_alloc")

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(lib().zkmi_h2d(self.ctx.h, self.ptr, arr.ctypes.data_as(vp), arr.nbytes), "zkmi_h2d")

    def download(self, arr: np.ndarray):
        assert arr.flags.c_contiguous and arr.nbytes <= self.nbytes
        check(lib().zkmi_d2h(self.ctx.h, arr.ctypes.data_as(vp), self.ptr, arr.nbytes), "zkmi_d2h")
        return arr

    def view(self, offset: int, nbytes: int) -> "DeviceView":
        """[offset, offset + nbytes) of this buffer (no ownership)."""
        assert 0 <= offset and offset + nbytes <= self.nbytes
        return DeviceView(self, offset, nbytes)

    def free(self):
        if self.ptr:
            lib().zkmi_dev_free(self.ctx.h, self.ptr)
            self.ptr = vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView(DeviceBuffer):
    """A sub-range of a DeviceBuffer (e.g. one batch's z in a multi-batch
    witness buffer); keeps its parent alive and never frees."""

    def __init__(self, parent: DeviceBuffer, offset: int, nbytes: int):
        self.ctx, self.nbytes, self.parent = parent.ctx, nbytes, parent
        self.ptr = vp(parent.ptr.value + offset)

    def free(self):
        self.ptr = vp()


class _Handle:
    """A native object made on a Context: `h` is its handle, `_destroy` names
    the entry point that frees it.  The context closes the objects it still
    tracks before it goes, so close() may run more than once."""
    _destroy = ""

    def _open(self, ctx: "Context"):
        self.h = vp()
        ctx._track(self)

    def close(self):
        if self.h:
            getattr(lib(), self._destroy)(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _positions(positions) -> np.ndarray:
    """tree positions for the C ABI: a contiguous u64 array"""
    return np.ascontiguousarray(np.asarray(list(positions), np.uint64))


def _outbuf(n: int, *shape, dtype=np.uint64) -> np.ndarray:
    """A zeroed output array of n rows of `shape`, never empty (the C ABI takes
    no null output pointer for n = 0): callers hand back its [:n]."""
    return np.zeros((max(n, 1),) + shape, dtype)


class Bases(_Handle):
    _destroy = "zkmi_bases_destroy"

    def __init__(self, ctx: "Context", points, g2: bool, *, generate_seed=None, n=None, first=0):
        self._open(ctx)
        if generate_seed is not None:
            self.ctx, self.g2, self.n = ctx, g2, n
            if first:
                assert not g2, "ranged generation is G1 only"
                check(lib().zkmi_bases_generate_range_g1(ctx.h, generate_seed, first, n, ctypes.byref(self.h)),
                      "zkmi_bases_generate_range_g1")
                return
            f = lib().zkmi_bases_generate_g2 if g2 else lib().zkmi_bases_generate_g1
            check(f(ctx.h, generate_seed, n, ctypes.byref(self.h)), "zkmi_bases_generate")
            return
        pts = np.ascontiguousarray(points, dtype=np.uint64)
        assert pts.ndim == 2 and pts.shape[1] == (16 if g2 else 8)
        self.ctx, self.g2, self.n = ctx, g2, pts.shape[0]
        f = lib().zkmi_bases_create_g2 if g2 else lib().zkmi_bases_create_g1
        check(f(ctx.h, _p64(pts), self.n, ctypes.byref(self.h)), "zkmi_bases_create")

    def precompute(self, c: int = 0, factor: int = 0):
        """Build the fixed-base table (see zkmi_bases_precompute); returns info()."""
        check(lib().zkmi_bases_precompute(self.h, c, factor), "zkmi_bases_precompute")
        return self.info()

    def info(self):
        """(len, table window or 0, copies, windows per copy)"""
        out = np.zeros(4, np.uint64)
        check(lib().zkmi_bases_info(self.h, _p64(out)), "zkmi_bases_info")
        return tuple(int(v) for v in out)

    def export(self):
        out = np.zeros((self.n, 16 if self.g2 else 8), np.uint64)
        check(lib().zkmi_bases_export(self.h, _p64(out)), "zkmi_bases_export")
        return out


class Context:
    def __init__(self, device: int = 0):
        self.h = vp()
        self.device = device
        # native objects made on this context (base sets, keys, R1CS, witness
        # programs, communicators): close() frees them first, so none outlives
        # the context it points to whatever order the garbage collector picks
        self._deps = weakref.WeakSet()
        check(lib().zkmi_ctx_create(device, ctypes.byref(self.h)), "zkmi_ctx_create")

    def _track(self, obj):
        self._deps.add(obj)
        return obj

    def close(self):
        if self.h:
            for obj in list(self._deps):
                try:
                    obj.close()
                except Exception:
                    pass
            lib().zkmi_ctx_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- timing
    def profile(self, on: bool = True):
        check(lib().zkmi_profile_enable(self.h, int(on)))

    def profile_get(self, name: str):
        t, c = ctypes.c_double(), ctypes.c_uint64()
        check(lib().zkmi_profile_get(self.h, name.encode(), ctypes.byref(t), ctypes.byref(c)))
        return t.value, c.value

    def profile_reset(self):
        check(lib().zkmi_profile_reset(self.h))

    def set_window(self, c: int):
        check(lib().zkmi_msm_set_window(self.h, c))

    def set_batch_group(self, g: int):
        """Proofs / MSMs per batched launch sequence (0 = automatic, 1..64)."""
        check(lib().zkmi_ctx_set_batch_group(self.h, g), "zkmi_ctx_set_batch_group")

    def batch_group(self) -> int:
        return lib().zkmi_ctx_get_batch_group(self.h)

    def set_prove_check(self, on: bool):
        """Proof jobs submitted while on also check their witness against the
        R1CS (groth16_last_check after the wait); off by default."""
        check(lib().zkmi_ctx_set_prove_check(self.h, int(bool(on))), "zkmi_ctx_set_prove_check")

    def prove_check(self) -> bool:
        return lib().zkmi_ctx_get_prove_check(self.h) == 1

    def set_verify_probes(self, n: int):
        """Probe budget of groth16_verify_many: 0 (default) = unlimited; n >= 1
        = at most n host final exponentiations, then the undecided proofs get
        exact verdicts on the GPU (groth16_verify_last reports them)."""
        check(lib().zkmi_ctx_set_verify_probes(self.h, int(n)), "zkmi_ctx_set_verify_probes")

    def get_verify_probes(self) -> int:
        return int(lib().zkmi_ctx_get_verify_probes(self.h))

    def set_lanes(self, lanes: int):
        """MSM lanes (capped at 2 while a communicator exists: stream budget)."""
        check(lib().zkmi_msm_set_lanes(self.h, lanes))

    def lanes(self) -> int:
        """MSM lanes in effect."""
        return lib().zkmi_msm_get_lanes(self.h)

    def stream_count(self) -> int:
        """Streams the library holds for this context (context, lanes,
        communicator and witness-program streams)."""
        return lib().zkmi_ctx_stream_count(self.h)

    def sync(self):
        check(lib().zkmi_sync(self.h))

    # --- MSM
    def bases_g1(self, points):
        return Bases(self, points, False)

    def bases_g2(self, points):
        return Bases(self, points, True)

    def bases_generate(self, seed: int, n: int, g2: bool = False, first: int = 0):
        """Synthetic bases k_i*G generated in HBM; elements [first, first+n) of seed's set."""
        return Bases(self, None, g2, generate_seed=seed, n=n, first=first)

    def bases_arith_g1(self, p0, d, n: int, first: int = 0):
        """Bases P_i = P0 + (first + i) * D generated in HBM (SURVEY.md §8d's
        point stream; P0, D canonical affine, 8 u64 each)."""
        b = Bases.__new__(Bases)
        b.ctx, b.g2, b.n = self, False, n
        b._open(self)
        p0 = np.ascontiguousarray(p0, np.uint64)
        d = np.ascontiguousarray(d, np.uint64)
        check(lib().zkmi_bases_generate_arith_g1(self.h, _p64(p0), _p64(d), first, n, ctypes.byref(b.h)),
              "zkmi_bases_generate_arith_g1")
        return b

    def scalars_upload(self, scalars: np.ndarray) -> DeviceBuffer:
        """(n, 4) canonical u64 scalars into a device buffer."""
        sc = np.ascontiguousarray(scalars, np.uint64).reshape(-1, 4)
        buf = DeviceBuffer(self, max(1, sc.shape[0]) * 32)
        if sc.shape[0]:
            buf.upload(sc)
        return buf

    def scalars_generate(self, seed: int, n: int, first: int = 0) -> DeviceBuffer:
        buf = DeviceBuffer(self, max(1, n) * 32)
        check(lib().zkmi_scalars_generate_range(self.h, seed, first, n, buf.ptr), "zkmi_scalars_generate_range")
        return buf

    def msm(self, bases: Bases, scalars, offset: int = 0):
        out = np.zeros(16 if bases.g2 else 8, np.uint64)
        if isinstance(scalars, DeviceBuffer):
            n = scalars.nbytes // 32
            f = lib().zkmi_msm_g2_device if bases.g2 else lib().zkmi_msm_g1_device
            check(f(self.h, bases.h, offset, scalars.ptr, n, _p64(out)), "zkmi_msm_device")
        else:
            sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
            f = lib().zkmi_msm_g2 if bases.g2 else lib().zkmi_msm_g1
            check(f(self.h, bases.h, offset, _p64(sc), sc.shape[0], _p64(out)), "zkmi_msm")
        return out

    def msm_submit(self, bases: Bases, dscalars: DeviceBuffer, n: int, offset: int = 0):
        """Queue an MSM; returns a job handle for msm_wait (host epilogue)."""
        job = vp()
        check(lib().zkmi_msm_submit(self.h, bases.h, offset, dscalars.ptr, n, ctypes.byref(job)), "zkmi_msm_submit")
        return (job, bases.g2)

    def msm_submit_shared(self, bases_list, dscalars: DeviceBuffer, n: int, offset: int = 0):
        """Queue MSMs of the same scalars over several base sets (one shared sort)."""
        k = len(bases_list)
        arr = (vp * k)(*[b.h for b in bases_list])
        jobs = (vp * k)()
        check(lib().zkmi_msm_submit_shared(self.h, arr, k, offset, dscalars.ptr, n, jobs), "zkmi_msm_submit_shared")
        return [(vp(jobs[i]), b.g2) for i, b in enumerate(bases_list)]

    def msm_wait(self, job):
        h, g2 = job
        out = np.zeros(16 if g2 else 8, np.uint64)
        check(lib().zkmi_msm_wait(h, _p64(out)), "zkmi_msm_wait")
        return out

    def msm_device_n(self, bases: Bases, dscalars: DeviceBuffer, n: int, offset: int = 0):
        out = np.zeros(16 if bases.g2 else 8, np.uint64)
        f = lib().zkmi_msm_g2_device if bases.g2 else lib().zkmi_msm_g1_device
        check(f(self.h, bases.h, offset, dscalars.ptr, n, _p64(out)), "zkmi_msm_device")
        return out

    def msm_batch_submit(self, bases: Bases, dscalars: DeviceBuffer, n: int, nb: int, stride: int, offset: int = 0):
        """Queue nb MSMs over one base set (vector i = n scalars at dscalars +
        i * stride bytes); finish with msm_batch_wait."""
        job = vp()
        check(lib().zkmi_msm_batch_submit(self.h, bases.h, offset, dscalars.ptr, n, nb, stride, ctypes.byref(job)),
              "zkmi_msm_batch_submit")
        return (job, bases.g2, nb)

    def msm_batch_wait(self, job):
        h, g2, nb = job
        out = np.zeros((nb, 16 if g2 else 8), np.uint64)
        check(lib().zkmi_msm_batch_wait(h, _p64(out), nb), "zkmi_msm_batch_wait")
        return out

    def msm_batch(self, bases: Bases, dscalars: DeviceBuffer, n: int, nb: int, stride: int, offset: int = 0):
        """(nb, 8 or 16) canonical affine results of nb MSMs over one base set."""
        return self.msm_batch_wait(self.msm_batch_submit(bases, dscalars, n, nb, stride, offset))

    # --- NTT
    def ntt(self, data: np.ndarray, log_n: int, inverse=False, coset=False):
        d = np.ascontiguousarray(data, dtype=np.uint64).copy()
        assert d.size == 4 << log_n
        check(lib().zkmi_ntt(self.h, _p64(d), log_n, int(inverse), int(coset)), "zkmi_ntt")
        return d.reshape(-1, 4)

    def ntt_device(self, buf: DeviceBuffer, log_n: int, inverse=False, coset=False):
        check(lib().zkmi_ntt_device(self.h, buf.ptr, log_n, int(inverse), int(coset)), "zkmi_ntt_device")

    def ntt_batch_device(self, buf: DeviceBuffer, log_n: int, nb: int, stride: int, inverse=False, coset=False):
        """nb in-place transforms, vector i at buf + i * stride bytes."""
        check(lib().zkmi_ntt_batch_device(self.h, buf.ptr, log_n, nb, stride, int(inverse), int(coset)),
              "zkmi_ntt_batch_device")


def shard_range(total: int, nranks: int, rank: int):
    """(first, count) of rank's contiguous point shard (zkmi_shard_range)."""
    f, c = ctypes.c_size_t(), ctypes.c_size_t()
    check(lib().zkmi_shard_range(total, nranks, rank, ctypes.byref(f), ctypes.byref(c)), "zkmi_shard_range")
    return f.value, c.value


def comm_unique_id() -> bytes:
    """RCCL unique id (one rank creates it, the host broadcasts it)."""
    buf = (ctypes.c_uint8 * 128)()
    check(lib().zkmi_comm_unique_id(buf), "zkmi_comm_unique_id")
    return bytes(buf)


class Comm(_Handle):
    """Multi-rank communicator of a context (zkmi.h multi-GPU section).

    Comm.rccl(ctx, uid, nranks, rank): RCCL transport (one rank per GPU).
    Comm.host(ctx, nranks, rank, allgather): host transport; `allgather(bytes)
    -> list[bytes]` of every rank (e.g. torch.distributed over gloo), for
    ranks that share a GPU or hosts without RCCL."""

    _destroy = "zkmi_comm_destroy"

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._cb = None
        self._open(ctx)

    @classmethod
    def rccl(cls, ctx: Context, uid: bytes, nranks: int, rank: int) -> "Comm":
        c = cls(ctx)
        ub = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        check(lib().zkmi_comm_init(ctx.h, ub, nranks, rank, ctypes.byref(c.h)), "zkmi_comm_init")
        return c

    @classmethod
    def host(cls, ctx: Context, nranks: int, rank: int, allgather) -> "Comm":
        from ._lib import ALLGATHER_FN

        c = cls(ctx)

        def cb(_user, send, recv, nbytes):
            try:
                parts = allgather(ctypes.string_at(send, nbytes))
                blob = b"".join(parts)
                assert len(blob) == nbytes * nranks
                ctypes.memmove(recv, blob, len(blob))
                return 0
            except Exception:  # reported to the caller as the entry point's error
                return 1

        c._cb = ALLGATHER_FN(cb)
        check(lib().zkmi_comm_init_host(ctx.h, nranks, rank, ctypes.cast(c._cb, vp), None, ctypes.byref(c.h)),
              "zkmi_comm_init_host")
        return c

    def info(self):
        """(nranks, rank, transport: 0 RCCL, 1 host)"""
        out = (ctypes.c_int * 3)()
        check(lib().zkmi_comm_info(self.h, out), "zkmi_comm_info")
        return tuple(out)

    def msm_submit(self, shard: "Bases", dscalars: "DeviceBuffer", n: int, offset: int = 0):
        job = vp()
        check(lib().zkmi_msm_sharded_submit(self.h, shard.h, offset, dscalars.ptr if n else None, n,
                                            ctypes.byref(job)), "zkmi_msm_sharded_submit")
        return (job, shard.g2)

    def msm(self, shard: "Bases", dscalars: "DeviceBuffer", n: int, offset: int = 0):
        return self.ctx.msm_wait(self.msm_submit(shard, dscalars, n, offset))

    def msm_windows_submit(self, bases: "Bases", dscalars: "DeviceBuffer", n: int, offset: int = 0):
        """Window-sharded MSM (zkmi_msm_window_sharded_submit): every rank
        passes the whole base set and scalars and runs its share of the plain
        plan's windows; every rank's wait returns the whole MSM."""
        job = vp()
        check(lib().zkmi_msm_window_sharded_submit(self.h, bases.h, offset, dscalars.ptr if n else None, n,
                                                   ctypes.byref(job)), "zkmi_msm_window_sharded_submit")
        return (job, bases.g2)

    def msm_windows(self, bases: "Bases", dscalars: "DeviceBuffer", n: int, offset: int = 0):
        return self.ctx.msm_wait(self.msm_windows_submit(bases, dscalars, n, offset))


def g1_add(a, b):
    out = np.zeros(8, np.uint64)
    check(lib().zkmi_g1_add(_p64(np.ascontiguousarray(a, np.uint64)), _p64(np.ascontiguousarray(b, np.uint64)),
                            _p64(out)))
    return out


def g2_add(a, b):
    out = np.zeros(16, np.uint64)
    check(lib().zkmi_g2_add(_p64(np.ascontiguousarray(a, np.uint64)), _p64(np.ascontiguousarray(b, np.uint64)),
                            _p64(out)))
    return out


def r1cs_struct(cs):
    """zelana_amd.r1cs.R1CS -> (ctypes R1CSStruct, keep-alive list)."""
    keep = []
    s = R1CSStruct()
    s.num_constraints, s.num_instance, s.num_witness = cs.num_constraints, cs.num_instance, cs.num_witness
    for name in ("a", "b", "c"):
        rp, col, val = cs.csr(name)
        keep += [rp, col, val]
        setattr(s, name + "_rowptr", rp.ctypes.data)
        setattr(s, name + "_col", col.ctypes.data)
        setattr(s, name + "_val", val.ctypes.data)
    return s, keep


class ProvingKey(_Handle):
    """arkworks ProvingKey<Bn254> resident on the GPU (zkmi_pk_load)."""
    _destroy = "zkmi_pk_destroy"

    def __init__(self, ctx: Context, pk_bytes: bytes, compressed: bool = True):
        self.ctx = ctx
        self._open(ctx)
        buf = np.frombuffer(pk_bytes, np.uint8)  # (read only: zkmi_pk_load takes a const pointer; no host copy)
        check(lib().zkmi_pk_load(ctx.h, buf.ctypes.data_as(u8p), len(pk_bytes), int(compressed),
                                 ctypes.byref(self.h)), "zkmi_pk_load")
        info = np.zeros(3, np.uint64)
        check(lib().zkmi_pk_info(self.h, _p64(info)))
        self.n, self.num_instance, self.num_witness = (int(x) for x in info)

    def precompute(self, factor: int = 0):
        """Fixed-base tables for all queries (zkmi_pk_precompute); proofs unchanged."""
        check(lib().zkmi_pk_precompute(self.h, factor), "zkmi_pk_precompute")
        return self

    def b_terms(self) -> int:
        """Variables the B-query MSMs run over (fewer than V - 1 once
        precompute() has dropped the ones whose B bases are at infinity)."""
        v = np.zeros(1, np.uint64)
        check(lib().zkmi_pk_b_terms(self.h, _p64(v)), "zkmi_pk_b_terms")
        return int(v[0])

    def vk_bytes(self) -> bytes:
        ln = ctypes.c_size_t()
        check(lib().zkmi_pk_vk_bytes(self.h, None, 0, ctypes.byref(ln)))
        buf = np.zeros(ln.value, np.uint8)
        check(lib().zkmi_pk_vk_bytes(self.h, buf.ctypes.data_as(u8p), ln.value, ctypes.byref(ln)))
        return buf.tobytes()

    def serialize(self) -> bytes:
        """ProvingKey::serialize_compressed (zkmi_pk_serialize)."""
        ln = ctypes.c_size_t()
        check(lib().zkmi_pk_serialize(self.h, None, 0, ctypes.byref(ln)), "zkmi_pk_serialize")
        buf = np.zeros(ln.value, np.uint8)
        check(lib().zkmi_pk_serialize(self.h, buf.ctypes.data_as(u8p), ln.value, ctypes.byref(ln)),
              "zkmi_pk_serialize")
        return buf.tobytes()

    @classmethod
    def setup(cls, ctx: "Context", cs, toxic: list[int], g1, g2) -> "ProvingKey":
        """zkmi_groth16_setup: toxic = [alpha, beta, gamma, delta, t], g1 / g2
        canonical affine generators (see zelana_amd/keygen.py for the RNG)."""
        st, keep = r1cs_struct(cs)
        tw = np.concatenate([_limbs(v) for v in toxic])
        pk = cls.__new__(cls)
        pk.ctx = ctx
        pk._open(ctx)
        check(lib().zkmi_groth16_setup(ctx.h, ctypes.byref(st), _p64(tw), _p64(np.ascontiguousarray(g1, np.uint64)),
                                       _p64(np.ascontiguousarray(g2, np.uint64)), ctypes.byref(pk.h)),
              "zkmi_groth16_setup")
        del keep
        info = np.zeros(3, np.uint64)
        check(lib().zkmi_pk_info(pk.h, _p64(info)))
        pk.n, pk.num_instance, pk.num_witness = (int(x) for x in info)
        return pk


def vk_canonical(ctx: Context, vk_bytes: bytes) -> bytes:
    """VerifyingKey::deserialize_compressed (validated on the GPU) re-serialized."""
    src = np.frombuffer(vk_bytes, np.uint8).copy()
    ln = ctypes.c_size_t()
    check(lib().zkmi_vk_canonical(ctx.h, src.ctypes.data_as(u8p), len(vk_bytes), None, 0, ctypes.byref(ln)),
          "Failed to deserialize verifying key")
    out = np.zeros(ln.value, np.uint8)
    check(lib().zkmi_vk_canonical(ctx.h, src.ctypes.data_as(u8p), len(vk_bytes), out.ctypes.data_as(u8p), ln.value,
                                  ctypes.byref(ln)), "Failed to deserialize verifying key")
    return out.tobytes()


def _limbs(x: int) -> np.ndarray:
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)


def groth16_prove(ctx: Context, pk: ProvingKey, cs, z: np.ndarray, r: int, s: int):
    """Canonical affine (A[8], B[16], C[8]) as numpy u64."""
    st, keep = r1cs_struct(cs)
    z = np.ascontiguousarray(z, np.uint64).reshape(-1, 4)
    a, b, c = np.zeros(8, np.uint64), np.zeros(16, np.uint64), np.zeros(8, np.uint64)
    rr, ss = _limbs(r), _limbs(s)
    check(lib().zkmi_groth16_prove(ctx.h, pk.h, ctypes.byref(st), _p64(z), _p64(rr), _p64(ss), _p64(a), _p64(b),
                                   _p64(c)), "zkmi_groth16_prove")
    del keep
    return a, b, c


def witness_map(ctx: Context, cs, z: np.ndarray) -> np.ndarray:
    st, keep = r1cs_struct(cs)
    z = np.ascontiguousarray(z, np.uint64).reshape(-1, 4)
    m, l = cs.num_constraints, cs.num_instance
    n = 1
    while n < m + l:
        n <<= 1
    h = np.zeros((n, 4), np.uint64)
    check(lib().zkmi_witness_map(ctx.h, ctypes.byref(st), _p64(z), _p64(h)), "zkmi_witness_map")
    del keep
    return h


def groth16_verify(vk_bytes: bytes, public_inputs, a, b, c) -> bool:
    """zkmi_groth16_verify (host pairing check of the on-chain verifier's
    relation; vk_bytes = arkworks-compressed VerifyingKey, inputs = ints)."""
    vk = np.frombuffer(bytes(vk_bytes), np.uint8).copy()
    ins = np.array([_limbs(int(x)) for x in public_inputs], np.uint64).reshape(-1, 4)
    ok = ctypes.c_int(0)
    check(lib().zkmi_groth16_verify(vk.ctypes.data_as(u8p), vk.size, _p64(ins), len(public_inputs),
                                    _p64(np.ascontiguousarray(a, np.uint64)), _p64(np.ascontiguousarray(b, np.uint64)),
                                    _p64(np.ascontiguousarray(c, np.uint64)), ctypes.byref(ok)), "zkmi_groth16_verify")
    return bool(ok.value)


class VerifyingKey(_Handle):
    """arkworks-compressed VerifyingKey decoded and validated once
    (zkmi_vk_load), for groth16_verify_many.  A bad key raises ZkmiError."""
    _destroy = "zkmi_vk_destroy"

    def __init__(self, ctx: Context, vk_bytes: bytes):
        self.ctx = ctx
        self._open(ctx)
        buf = np.frombuffer(bytes(vk_bytes), np.uint8)
        check(lib().zkmi_vk_load(ctx.h, buf.ctypes.data_as(u8p), buf.size, ctypes.byref(self.h)), "zkmi_vk_load")
        info = np.zeros(1, np.uint64)
        check(lib().zkmi_vk_info(self.h, _p64(info)), "zkmi_vk_info")
        self.n_inputs = int(info[0])


def groth16_verify_many(ctx: Context, vk: VerifyingKey, proofs, inputs, rho=None):
    """zkmi_groth16_verify_many: proofs = [(a, b, c), ...] canonical points,
    inputs = one list of ints per proof (vk.n_inputs each).  rho: None = the
    library draws the 128-bit weights itself (the sound use); a list of
    non-zero ints < 2^128 fixes them (tests).  Returns ([bool per proof],
    {"pairs", "final_exps", "invalid_points"})."""
    nb = len(proofs)
    a, b, c, ins = _proof_arrays(vk, proofs, inputs)
    if rho is not None and len(rho) != nb:
        raise ValueError("one weight per proof")
    w = None
    if rho is not None:
        if any(not 0 <= int(v) < 1 << 128 for v in rho):
            raise ValueError("weights are 128-bit values")
        w = np.array([[int(v) & (2**64 - 1), int(v) >> 64] for v in rho], np.uint64).reshape(nb, 2)
    valid = _outbuf(nb, dtype=np.uint8)
    st = VerifyStatsStruct()
    check(lib().zkmi_groth16_verify_many(ctx.h, vk.h, nb, _p64(ins), _p64(a), _p64(b), _p64(c),
                                         None if w is None else _p64(w), valid.ctypes.data_as(u8p), ctypes.byref(st)),
          "zkmi_groth16_verify_many")
    return [bool(v) for v in valid[:nb]], {"pairs": int(st.pairs), "final_exps": int(st.final_exps),
                                           "invalid_points": int(st.invalid_points)}


def _proof_arrays(vk, proofs, inputs):
    nb = len(proofs)
    if len(inputs) != nb or any(len(x) != vk.n_inputs for x in inputs):
        raise ValueError(f"{nb} proofs need {nb} x {vk.n_inputs} public inputs")
    a = np.ascontiguousarray([np.asarray(p[0], np.uint64) for p in proofs], np.uint64).reshape(nb, 8)
    b = np.ascontiguousarray([np.asarray(p[1], np.uint64) for p in proofs], np.uint64).reshape(nb, 16)
    c = np.ascontiguousarray([np.asarray(p[2], np.uint64) for p in proofs], np.uint64).reshape(nb, 8)
    ins = np.array([[_limbs(int(v)) for v in x] for x in inputs], np.uint64).reshape(nb, vk.n_inputs, 4)
    return a, b, c, ins


def groth16_verify_each(ctx: Context, vk: VerifyingKey, proofs, inputs):
    """zkmi_groth16_verify_each: exact per-proof verdicts, Miller loops and
    final exponentiations on the GPU (no weights, no soundness error; the cost
    does not depend on how many proofs are bad).  Arguments as
    groth16_verify_many's.  Returns ([bool per proof], {"pairs", "final_exps",
    "invalid_points"})."""
    nb = len(proofs)
    a, b, c, ins = _proof_arrays(vk, proofs, inputs)
    valid = _outbuf(nb, dtype=np.uint8)
    st = VerifyStatsStruct()
    check(lib().zkmi_groth16_verify_each(ctx.h, vk.h, nb, _p64(ins), _p64(a), _p64(b), _p64(c),
                                         valid.ctypes.data_as(u8p), ctypes.byref(st)), "zkmi_groth16_verify_each")
    return [bool(v) for v in valid[:nb]], {"pairs": int(st.pairs), "final_exps": int(st.final_exps),
                                           "invalid_points": int(st.invalid_points)}


def groth16_verify_last(ctx: Context) -> dict:
    """zkmi_groth16_verify_last: what the last groth16_verify_many handed to
    the GPU when its probe budget ran out (all 0 when it was not hit)."""
    out = np.zeros(3, np.uint64)
    check(lib().zkmi_groth16_verify_last(ctx.h, _p64(out)), "zkmi_groth16_verify_last")
    return {"gpu_decided": int(out[0]), "gpu_pairs": int(out[1]), "gpu_final_exps": int(out[2])}


def proof_to_alt_bn128_bytes(a, b, c) -> bytes:
    """-A || B || C in the alt_bn128 syscalls' big-endian encoding."""
    out = np.zeros(256, np.uint8)
    check(lib().zkmi_proof_to_alt_bn128_bytes(_p64(np.ascontiguousarray(a, np.uint64)),
                                              _p64(np.ascontiguousarray(b, np.uint64)),
                                              _p64(np.ascontiguousarray(c, np.uint64)), out.ctypes.data_as(u8p)))
    return out.tobytes()


def proof_to_solana_bytes(a, b, c) -> bytes:
    out = np.zeros(256, np.uint8)
    check(lib().zkmi_proof_to_solana_bytes(_p64(np.ascontiguousarray(a, np.uint64)),
                                           _p64(np.ascontiguousarray(b, np.uint64)),
                                           _p64(np.ascontiguousarray(c, np.uint64)), out.ctypes.data_as(u8p)))
    return out.tobytes()


def proof_serialize_compressed(a, b, c) -> bytes:
    out = np.zeros(128, np.uint8)
    check(lib().zkmi_proof_serialize_compressed(_p64(np.ascontiguousarray(a, np.uint64)),
                                                _p64(np.ascontiguousarray(b, np.uint64)),
                                                _p64(np.ascontiguousarray(c, np.uint64)), out.ctypes.data_as(u8p)))
    return out.tobytes()


PROOF_ARK_COMPRESSED, PROOF_ARK_UNCOMPRESSED, PROOF_SOLANA_LE, PROOF_ALT_BN128_BE = 0, 1, 2, 3  # ZKMI_PROOF_*
PROOF_FORMATS = {"compressed": PROOF_ARK_COMPRESSED, "uncompressed": PROOF_ARK_UNCOMPRESSED,
                 "solana": PROOF_SOLANA_LE, "alt_bn128": PROOF_ALT_BN128_BE}


class ProofDecodeError(ValueError):
    """proof_decode: status 1 = malformed encoding, 2 = a well-formed encoding
    of an invalid point (off the curve / twist, or B outside the subgroup)."""

    def __init__(self, status: int, msg: str):
        super().__init__(msg)
        self.status = status


def proof_encoded_len(fmt: int) -> int:
    n = int(lib().zkmi_proof_encoded_len(fmt))
    if not n:
        raise ValueError(f"unknown proof format {fmt}")
    return n


def _encoded(fmt: int, raws):
    """bytes (nb encodings back to back) or a list of bytes -> (u8 array, nb)"""
    n = proof_encoded_len(fmt)
    if isinstance(raws, (bytes, bytearray, memoryview)):
        buf = bytes(raws)
        if len(buf) % n:
            raise ValueError(f"{len(buf)} bytes are no whole number of {n}-byte proofs")
    else:
        raws = [bytes(r) for r in raws]
        if any(len(r) != n for r in raws):
            raise ValueError(f"every proof of format {fmt} takes {n} bytes")
        buf = b"".join(raws)
    return np.frombuffer(buf, np.uint8), len(buf) // n


def proof_decode(fmt: int, raw: bytes):
    """zkmi_proof_decode (host): one encoded proof -> canonical (a, b, c).
    Raises ProofDecodeError (status 1 malformed, wrong length included; 2
    invalid point)."""
    buf = np.frombuffer(bytes(raw), np.uint8)
    a, b, c = np.zeros(8, np.uint64), np.zeros(16, np.uint64), np.zeros(8, np.uint64)
    rc = lib().zkmi_proof_decode(fmt, buf.ctypes.data_as(u8p), buf.size, _p64(a), _p64(b), _p64(c))
    if rc:
        status = 2 if rc == -5 else 1  # ZKMI_EPOINT: an invalid point; anything else: malformed
        raise ProofDecodeError(status, lib().zkmi_last_error().decode(errors="replace"))
    return a, b, c


def proofs_decode(ctx: Context, fmt: int, raws):
    """zkmi_proofs_decode: encoded proofs (bytes back to back, or a list of
    bytes) decoded and validated on the GPU.  Returns (a[nb, 8], b[nb, 16],
    c[nb, 8], status[nb]): status 0 ok, 1 malformed, 2 invalid point; the rows
    of a non-ok proof are zero."""
    buf, nb = _encoded(fmt, raws)
    a, b, c = np.zeros((nb, 8), np.uint64), np.zeros((nb, 16), np.uint64), np.zeros((nb, 8), np.uint64)
    status = _outbuf(nb, dtype=np.uint8)
    check(lib().zkmi_proofs_decode(ctx.h, fmt, buf.ctypes.data_as(u8p), nb, _p64(a), _p64(b), _p64(c),
                                   status.ctypes.data_as(u8p)), "zkmi_proofs_decode")
    return a, b, c, status[:nb]


def _input_array(vk, nb, inputs):
    """one list of ints per proof, or canonical limbs already (nb, n_inputs, 4) u64"""
    if isinstance(inputs, np.ndarray):
        ins = np.ascontiguousarray(inputs, np.uint64)
        if ins.shape != (nb, vk.n_inputs, 4):
            raise ValueError(f"{nb} proofs need public inputs of shape ({nb}, {vk.n_inputs}, 4)")
        return ins
    if len(inputs) != nb or any(len(x) != vk.n_inputs for x in inputs):
        raise ValueError(f"{nb} proofs need {nb} x {vk.n_inputs} public inputs")
    return np.array([[_limbs(int(v)) for v in x] for x in inputs], np.uint64).reshape(nb, vk.n_inputs, 4)


def _stats(st) -> dict:
    return {"pairs": int(st.pairs), "final_exps": int(st.final_exps), "invalid_points": int(st.invalid_points)}


def groth16_verify_many_encoded(ctx: Context, vk: VerifyingKey, fmt: int, raws, inputs, rho=None):
    """zkmi_groth16_verify_many_encoded: groth16_verify_many over encoded
    proofs (bytes back to back, or a list of bytes), decoded on the GPU.
    inputs: one list of ints per proof, or a (nb, n_inputs, 4) u64 array of
    canonical limbs.  Returns ([bool per proof], [malformed per proof], stats);
    a malformed proof is False and counts in stats["invalid_points"]."""
    buf, nb = _encoded(fmt, raws)
    ins = _input_array(vk, nb, inputs)
    w = None
    if rho is not None:
        if len(rho) != nb or any(not 0 <= int(v) < 1 << 128 for v in rho):
            raise ValueError("one 128-bit weight per proof")
        w = np.array([[int(v) & (2**64 - 1), int(v) >> 64] for v in rho], np.uint64).reshape(nb, 2)
    valid, mal = _outbuf(nb, dtype=np.uint8), _outbuf(nb, dtype=np.uint8)
    st = VerifyStatsStruct()
    check(lib().zkmi_groth16_verify_many_encoded(ctx.h, vk.h, fmt, nb, buf.ctypes.data_as(u8p), _p64(ins),
                                                 None if w is None else _p64(w), valid.ctypes.data_as(u8p),
                                                 mal.ctypes.data_as(u8p), ctypes.byref(st)),
          "zkmi_groth16_verify_many_encoded")
    return [bool(v) for v in valid[:nb]], [bool(v) for v in mal[:nb]], _stats(st)


def groth16_verify_each_encoded(ctx: Context, vk: VerifyingKey, fmt: int, raws, inputs):
    """zkmi_groth16_verify_each_encoded: groth16_verify_each over encoded
    proofs; arguments and results as groth16_verify_many_encoded's."""
    buf, nb = _encoded(fmt, raws)
    ins = _input_array(vk, nb, inputs)
    valid, mal = _outbuf(nb, dtype=np.uint8), _outbuf(nb, dtype=np.uint8)
    st = VerifyStatsStruct()
    check(lib().zkmi_groth16_verify_each_encoded(ctx.h, vk.h, fmt, nb, buf.ctypes.data_as(u8p), _p64(ins),
                                                 valid.ctypes.data_as(u8p), mal.ctypes.data_as(u8p),
                                                 ctypes.byref(st)), "zkmi_groth16_verify_each_encoded")
    return [bool(v) for v in valid[:nb]], [bool(v) for v in mal[:nb]], _stats(st)


class R1CSDevice(_Handle):
    """Circuit matrices resident in HBM (zkmi_r1cs_create)."""
    _destroy = "zkmi_r1cs_destroy"

    def __init__(self, ctx: Context, cs):
        self.ctx = ctx
        st, keep = r1cs_struct(cs)
        self._open(ctx)
        check(lib().zkmi_r1cs_create(ctx.h, ctypes.byref(st), ctypes.byref(self.h)), "zkmi_r1cs_create")
        self.num_variables = cs.num_instance + cs.num_witness
        del keep


@dataclass
class R1CSStatus:
    """zkmi_r1cs_status: first_row is the lowest row with <a,z><b,z> != <c,z>
    (None if every row holds), n_bad the number of such rows, a / b / c the
    three canonical values at first_row (0 if none)."""
    first_row: int | None
    n_bad: int
    a: int
    b: int
    c: int

    @property
    def ok(self) -> bool:
        return self.first_row is None


def _statuses(arr, count: int) -> list[R1CSStatus]:
    def val(w):
        return sum(int(w[k]) << (64 * k) for k in range(4))

    return [R1CSStatus(None if arr[i].first_row == ROW_NONE else int(arr[i].first_row), int(arr[i].n_bad),
                       val(arr[i].a), val(arr[i].b), val(arr[i].c)) for i in range(count)]


def r1cs_check(ctx: Context, r1cs: R1CSDevice, dz: DeviceBuffer, nb: int = 1, stride: int | None = None):
    """Row satisfaction of nb resident assignments (assignment i at dz + i *
    stride bytes, default packed) against a resident R1CS: [R1CSStatus]."""
    if stride is None:
        stride = r1cs.num_variables * 32
    out = (R1CSStatusStruct * max(1, nb))()
    check(lib().zkmi_r1cs_check(ctx.h, r1cs.h, dz.ptr, nb, stride, out), "zkmi_r1cs_check")
    return _statuses(out, nb)


def groth16_last_check(ctx: Context) -> list[R1CSStatus]:
    """Statuses of the proofs of the proof job most recently waited on ctx, in
    proof order; [] if it was submitted with the check off."""
    cnt = ctypes.c_size_t()
    lib().zkmi_groth16_last_check(ctx.h, None, 0, ctypes.byref(cnt))  # (EINVAL when there are any: count only)
    out = (R1CSStatusStruct * max(1, cnt.value))()
    check(lib().zkmi_groth16_last_check(ctx.h, out, cnt.value, ctypes.byref(cnt)), "zkmi_groth16_last_check")
    return _statuses(out, cnt.value)


def synthetic_pk(ctx: Context, seed: int, log_n: int, num_instance: int, num_witness: int) -> "ProvingKey":
    """Random proving key of the given shape generated in HBM (benchmarks)."""
    pk = ProvingKey.__new__(ProvingKey)
    pk.ctx = ctx
    pk.h = vp()
    check(lib().zkmi_pk_synthetic(ctx.h, seed, log_n, num_instance, num_witness, ctypes.byref(pk.h)),
          "zkmi_pk_synthetic")
    pk.n, pk.num_instance, pk.num_witness = 1 << log_n, num_instance, num_witness
    return pk


def groth16_prove_submit(ctx: Context, pk: "ProvingKey", r1cs: R1CSDevice, dz: DeviceBuffer, r: int, s: int):
    """Queue a resident proof (zkmi_groth16_prove_submit); finish with groth16_prove_wait."""
    job = vp()
    check(lib().zkmi_groth16_prove_submit(ctx.h, pk.h, r1cs.h, dz.ptr, _p64(_limbs(r)), _p64(_limbs(s)),
                                          ctypes.byref(job)), "zkmi_groth16_prove_submit")
    return job


def groth16_prove_wait(job):
    a, b, c = np.zeros(8, np.uint64), np.zeros(16, np.uint64), np.zeros(8, np.uint64)
    check(lib().zkmi_groth16_prove_wait(job, _p64(a), _p64(b), _p64(c)), "zkmi_groth16_prove_wait")
    return a, b, c


def groth16_prove_resident(ctx: Context, pk: "ProvingKey", r1cs: R1CSDevice, dz: DeviceBuffer, r: int, s: int):
    a, b, c = np.zeros(8, np.uint64), np.zeros(16, np.uint64), np.zeros(8, np.uint64)
    check(lib().zkmi_groth16_prove_resident(ctx.h, pk.h, r1cs.h, dz.ptr, _p64(_limbs(r)), _p64(_limbs(s)), _p64(a),
                                            _p64(b), _p64(c)), "zkmi_groth16_prove_resident")
    return a, b, c


def _limbs_many(xs) -> np.ndarray:
    return np.array([_limbs(int(x)) for x in xs], np.uint64).reshape(-1, 4)


def groth16_prove_many_submit(ctx: Context, pk: "ProvingKey", r1cs: R1CSDevice, dz: DeviceBuffer, nb: int,
                              stride: int, rs, ss):
    """Queue nb resident proofs of same-shape witnesses (assignment i at dz +
    i * stride bytes, blinding rs[i], ss[i]); finish with groth16_prove_many_wait."""
    assert len(rs) == nb and len(ss) == nb
    job = vp()
    rr, sv = _limbs_many(rs), _limbs_many(ss)
    check(lib().zkmi_groth16_prove_many_submit(ctx.h, pk.h, r1cs.h, dz.ptr, nb, stride, _p64(rr), _p64(sv),
                                               ctypes.byref(job)), "zkmi_groth16_prove_many_submit")
    return (job, nb)


def groth16_prove_many_wait(job):
    """[(A[8], B[16], C[8])] in submission order."""
    h, nb = job
    a, b, c = np.zeros((nb, 8), np.uint64), np.zeros((nb, 16), np.uint64), np.zeros((nb, 8), np.uint64)
    check(lib().zkmi_groth16_prove_many_wait(h, nb, _p64(a), _p64(b), _p64(c)), "zkmi_groth16_prove_many_wait")
    return [(a[i], b[i], c[i]) for i in range(nb)]


def groth16_prove_many(ctx: Context, pk: "ProvingKey", r1cs: R1CSDevice, dz: DeviceBuffer, nb: int, stride: int,
                       rs, ss):
    return groth16_prove_many_wait(groth16_prove_many_submit(ctx, pk, r1cs, dz, nb, stride, rs, ss))



def _fe_words(vals, width: int = 1) -> np.ndarray:
    """field elements for the C ABI: an (n, 4 * width) u64 array as it is, or
    ints / 32-byte strings (any 256-bit value: the library takes them mod r)"""
    if isinstance(vals, np.ndarray) and vals.dtype == np.uint64:
        return np.ascontiguousarray(vals).reshape(-1, 4 * width)
    raw = b"".join(int(v).to_bytes(32, "little") if isinstance(v, int) else bytes(v) for v in vals)
    if len(raw) % (32 * width):
        raise ValueError("field elements are 32 bytes each")
    return np.frombuffer(raw, np.uint64).reshape(-1, 4 * width).copy()


def _hash_many(self, fn_name: str, tuples, arity: int | None) -> np.ndarray:
    """hash_many of a resident hasher (fn_name: its entry point): one hash per
    tuple, as an (n, 4) u64 array.  tuples: an (n, 4 * arity) u64 array (arity
    given), or equally long sequences of ints / 32-byte strings."""
    if arity is None:
        tuples = [tuple(t) for t in tuples]
        arity = len(tuples[0]) if tuples else 1
        if any(len(t) != arity for t in tuples):
            raise ValueError("hash_many: tuples of one length")
        tuples = [x for t in tuples for x in t]
    ins = _fe_words(tuples, arity)
    n = ins.shape[0]
    out = _outbuf(n, 4)
    check(getattr(lib(), fn_name)(self.ctx.h, self.h, n, arity, _p64(ins), _p64(out)), fn_name)
    return out[:n]


class PoseidonHasher(_Handle):
    """Resident constants of one Poseidon parameter set (zkmi_poseidon_create):
    width 3, x^5, `params` as l2block.poseidon_params gives them."""
    _destroy = "zkmi_poseidon_destroy"

    def __init__(self, ctx: Context, params):
        if params["rate"] != 2 or params["capacity"] != 1 or params["alpha"] != 5:
            raise ValueError("PoseidonHasher: rate 2, capacity 1, x^5 only")
        self.ctx, self.params = ctx, params
        self._open(ctx)
        table = _fe_words([int(c) for row in params["ark"] for c in row] + [int(c) for row in params["mds"] for c in row])
        check(lib().zkmi_poseidon_create(ctx.h, params["full"], params["partial"], _p64(table), ctypes.byref(self.h)),
              "zkmi_poseidon_create")

    def hash_many(self, tuples, arity: int | None = None) -> np.ndarray:
        """zkmi_poseidon_hash_many: one sponge hash per tuple (see _hash_many)."""
        return _hash_many(self, "zkmi_poseidon_hash_many", tuples, arity)


class NoteTreeDevice(_Handle):
    """An append-only Merkle tree over a PoseidonHasher, resident in HBM
    (zkmi_note_tree_create).  Arrays are (n, 4) u64 canonical words."""
    _destroy = "zkmi_note_tree_destroy"

    def __init__(self, ctx: Context, hasher: PoseidonHasher, depth: int, capacity: int, empty_leaf):
        self.ctx, self.hasher, self.depth, self.capacity = ctx, hasher, depth, capacity
        self._open(ctx)
        check(lib().zkmi_note_tree_create(ctx.h, hasher.h, depth, capacity, _p64(_fe_words([empty_leaf])),
                                          ctypes.byref(self.h)), "zkmi_note_tree_create")

    @property
    def next_position(self) -> int:
        info = np.zeros(3, np.uint64)
        check(lib().zkmi_note_tree_info(self.h, _p64(info)), "zkmi_note_tree_info")
        return int(info[2])

    def append(self, leaves, want_roots: bool = True):
        """-> (first position, (n, 4) per-insertion roots or None)"""
        lv = _fe_words(leaves)
        n = lv.shape[0]
        first = ctypes.c_uint64(0)
        roots = _outbuf(n, 4) if want_roots else None
        check(lib().zkmi_note_tree_append(self.ctx.h, self.h, n, _p64(lv), ctypes.byref(first),
                                          None if roots is None else _p64(roots)), "zkmi_note_tree_append")
        return int(first.value), None if roots is None else roots[:n]

    def root(self) -> np.ndarray:
        out = np.zeros(4, np.uint64)
        check(lib().zkmi_note_tree_root(self.ctx.h, self.h, _p64(out)), "zkmi_note_tree_root")
        return out

    def paths(self, positions) -> np.ndarray:
        """-> (n, depth, 4) siblings, the leaf level first"""
        pos = _positions(positions)
        out = _outbuf(pos.size, self.depth, 4)
        check(lib().zkmi_note_tree_paths(self.ctx.h, self.h, pos.size, _p64(pos), _p64(out)), "zkmi_note_tree_paths")
        return out[:pos.size]

    def leaves(self, first: int, n: int) -> np.ndarray:
        out = _outbuf(n, 4)
        check(lib().zkmi_note_tree_leaves(self.ctx.h, self.h, first, n, _p64(out)), "zkmi_note_tree_leaves")
        return out[:n]


class MimcHasher(_Handle):
    """Resident MiMC round constants (zkmi_mimc_create): the zelana_batch
    circuit's hash_1 .. hash_4, one lane per hash."""
    _destroy = "zkmi_mimc_destroy"

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._open(ctx)
        check(lib().zkmi_mimc_create(ctx.h, ctypes.byref(self.h)), "zkmi_mimc_create")

    def hash_many(self, tuples, arity: int | None = None) -> np.ndarray:
        """zkmi_mimc_hash_many: hash_arity of every tuple (see _hash_many)."""
        return _hash_many(self, "zkmi_mimc_hash_many", tuples, arity)


class AccountTreeDevice(_Handle):
    """The sparse MiMC account tree, resident in HBM (zkmi_account_tree_create):
    any position below 2^depth, a node store of max_nodes slots.  Arrays are
    (n, 4) u64 canonical words."""
    _destroy = "zkmi_account_tree_destroy"

    def __init__(self, ctx: Context, hasher: MimcHasher, depth: int, max_nodes: int):
        self.ctx, self.hasher, self.depth, self.max_nodes = ctx, hasher, depth, max_nodes
        self._open(ctx)
        check(lib().zkmi_account_tree_create(ctx.h, hasher.h, depth, max_nodes, ctypes.byref(self.h)),
              "zkmi_account_tree_create")

    @property
    def node_count(self) -> int:
        info = np.zeros(3, np.uint64)
        check(lib().zkmi_account_tree_info(self.h, _p64(info)), "zkmi_account_tree_info")
        return int(info[2])

    def apply(self, positions, leaves):
        """K ordered leaf writes -> ((K, depth, 4) siblings as write k sees
        them, (K, 4) replaced leaves, (K, 4) roots after each write)"""
        pos = _positions(positions)
        lv = _fe_words(leaves)
        if lv.shape[0] != pos.size:
            raise ValueError("apply: one leaf per position")
        k = pos.size
        sib = _outbuf(k, self.depth, 4)
        old, roots = _outbuf(k, 4), _outbuf(k, 4)
        check(lib().zkmi_account_tree_apply(self.ctx.h, self.h, k, _p64(pos), _p64(lv), _p64(sib), _p64(old),
                                            _p64(roots)), "zkmi_account_tree_apply")
        return sib[:k], old[:k], roots[:k]

    def root(self) -> np.ndarray:
        out = np.zeros(4, np.uint64)
        check(lib().zkmi_account_tree_root(self.ctx.h, self.h, _p64(out)), "zkmi_account_tree_root")
        return out

    def paths(self, positions) -> np.ndarray:
        """-> (n, depth, 4) siblings against the current state, the leaf level first"""
        pos = _positions(positions)
        out = _outbuf(pos.size, self.depth, 4)
        check(lib().zkmi_account_tree_paths(self.ctx.h, self.h, pos.size, _p64(pos), _p64(out)),
              "zkmi_account_tree_paths")
        return out[:pos.size]

    def leaves(self, positions) -> np.ndarray:
        pos = _positions(positions)
        out = _outbuf(pos.size, 4)
        check(lib().zkmi_account_tree_leaves(self.ctx.h, self.h, pos.size, _p64(pos), _p64(out)),
              "zkmi_account_tree_leaves")
        return out[:pos.size]


def _key_bytes(keys) -> np.ndarray:
    """32-byte keys for the C ABI: an (n, 32) u8 array as it is, an (n, 4) u64
    array, or a sequence of 32-byte strings / ints (little-endian, below
    2^256).  Keys are raw bytes: nothing is reduced mod r."""
    if isinstance(keys, np.ndarray) and keys.dtype == np.uint8:
        return np.ascontiguousarray(keys).reshape(-1, 32)
    if isinstance(keys, np.ndarray) and keys.dtype == np.uint64:
        return np.ascontiguousarray(keys).reshape(-1, 4).view(np.uint8).reshape(-1, 32)
    raw = b"".join(int(k).to_bytes(32, "little") if isinstance(k, int) else bytes(k) for k in keys)
    if len(raw) % 32:
        raise ValueError("keys are 32 bytes each")
    return np.frombuffer(raw, np.uint8).reshape(-1, 32)


NF_ACCEPTED, NF_SKIPPED, NF_SPENT_STORED, NF_SPENT_IN_CALL, NF_DUP_IN_TX = 0, 1, 2, 3, 4  # ZKMI_NF_*


class NullifierSetDevice(_Handle):
    """The spent-nullifier set, resident in HBM (zkmi_nullifier_set_create): at
    most `capacity` keys of 32 raw bytes, compared bytewise, kept in insertion
    order."""
    _destroy = "zkmi_nullifier_set_destroy"

    def __init__(self, ctx: Context, capacity: int):
        self.ctx, self.capacity = ctx, capacity
        self._open(ctx)
        check(lib().zkmi_nullifier_set_create(ctx.h, capacity, ctypes.byref(self.h)), "zkmi_nullifier_set_create")

    def info(self):
        """(capacity, slots of the table, keys stored)"""
        out = np.zeros(3, np.uint64)
        check(lib().zkmi_nullifier_set_info(self.h, _p64(out)), "zkmi_nullifier_set_info")
        return tuple(int(v) for v in out)

    @property
    def count(self) -> int:
        return self.info()[2]

    def contains(self, keys) -> list:
        """[bool per key]"""
        kb = _key_bytes(keys)
        n = kb.shape[0]
        out = _outbuf(n, dtype=np.uint8)
        check(lib().zkmi_nullifier_set_contains(self.ctx.h, self.h, n, kb.ctypes.data_as(u8p), out.ctypes.data_as(u8p)),
              "zkmi_nullifier_set_contains")
        return out[:n].astype(bool).tolist()

    def spend(self, keys, per_tx: int, eligible=None):
        """zkmi_nullifier_set_spend: len(keys) / per_tx transfers in order ->
        ([verdict per transfer] (NF_*), [detail per transfer], rounds).
        eligible: None = all, else one truth value per transfer."""
        kb = _key_bytes(keys)
        if per_tx < 1 or kb.shape[0] % per_tx:
            raise ValueError("spend: per_tx keys per transfer")
        ntx = kb.shape[0] // per_tx
        el = None
        if eligible is not None:
            el = np.ascontiguousarray([1 if e else 0 for e in eligible], np.uint8)
            if el.size != ntx:
                raise ValueError("spend: one eligible flag per transfer")
        verdict, detail = _outbuf(ntx, dtype=np.uint32), _outbuf(ntx, dtype=np.uint32)
        rounds = ctypes.c_uint32(0)
        check(lib().zkmi_nullifier_set_spend(self.ctx.h, self.h, ntx, per_tx, kb.ctypes.data_as(u8p),
                                             None if el is None else el.ctypes.data_as(u8p),
                                             verdict.ctypes.data_as(u32p), detail.ctypes.data_as(u32p),
                                             ctypes.byref(rounds)), "zkmi_nullifier_set_spend")
        return verdict[:ntx].tolist(), detail[:ntx].tolist(), int(rounds.value)

    def load(self, keys):
        """Restore from a persisted list (ShieldedState::load): spend with one
        key per transfer and no mask, so duplicates collapse."""
        return self.spend(keys, 1)

    def log(self, first: int, n: int) -> list:
        """the keys [first, first + n) in insertion order, as 32-byte strings"""
        out = _outbuf(n, 32, dtype=np.uint8)
        check(lib().zkmi_nullifier_set_log(self.ctx.h, self.h, first, n, out.ctypes.data_as(u8p)),
              "zkmi_nullifier_set_log")
        return [out[i].tobytes() for i in range(n)]


SCAN_NOT_MINE, SCAN_MALFORMED, SCAN_WRONG_COMMITMENT, SCAN_HIT = 0, 1, 2, 3  # ZKMI_SCAN_*
COMMIT_NONE, COMMIT_MIMC, COMMIT_POSEIDON = 0, 1, 2                         # ZKMI_COMMIT_*


@dataclass
class ScannedNote:
    """One note found by a scan.  memo is the raw bytes the sender declared."""
    position: int
    commitment: bytes
    value: int
    randomness: bytes
    memo: bytes


class NoteStoreDevice(_Handle):
    """The encrypted notes of a pool, resident in HBM (zkmi_note_store_create):
    at most `capacity` notes whose ciphertexts, tag included, are at most
    max_ct bytes; append-only.  hashers: mimc= a MimcHasher for COMMIT_MIMC
    scans, poseidon= a PoseidonHasher for COMMIT_POSEIDON ones."""
    _destroy = "zkmi_note_store_destroy"

    def __init__(self, ctx: Context, capacity: int, max_ct: int = 570, mimc=None, poseidon=None):
        self.ctx, self.capacity, self.max_ct, self.mimc, self.poseidon = ctx, capacity, max_ct, mimc, poseidon
        self._open(ctx)
        check(lib().zkmi_note_store_create(ctx.h, capacity, max_ct, ctypes.byref(self.h)), "zkmi_note_store_create")

    def info(self):
        """(capacity, max_ct, notes stored, ciphertext bytes stored)"""
        out = np.zeros(4, np.uint64)
        check(lib().zkmi_note_store_info(self.h, _p64(out)), "zkmi_note_store_info")
        return tuple(int(v) for v in out)

    @property
    def count(self) -> int:
        return self.info()[2]

    def append(self, notes):
        """notes: [(position, commitment, ephemeral_pk, nonce, ciphertext)],
        stored in this order.  Raises ZkmiError, with nothing stored, for a
        ciphertext above max_ct, a repeated position or a full store."""
        notes = list(notes)
        n = len(notes)
        if any(len(bytes(e)) != 32 or len(bytes(nc)) != 12 for _, _, e, nc, _ in notes):
            raise ValueError("append: 32-byte ephemeral keys and 12-byte nonces")
        pos = np.ascontiguousarray([p for p, *_ in notes], np.uint32).reshape(-1)
        cm = _key_bytes([c for _, c, *_ in notes])
        epk = np.frombuffer(b"".join(bytes(e) for _, _, e, _, _ in notes), np.uint8)
        nonce = np.frombuffer(b"".join(bytes(nc) for _, _, _, nc, _ in notes), np.uint8)
        lens = np.ascontiguousarray([len(ct) for *_, ct in notes], np.uint32).reshape(-1)
        cts = np.frombuffer(b"".join(bytes(ct) for *_, ct in notes) or b"\0", np.uint8)
        check(lib().zkmi_note_store_append(self.ctx.h, self.h, n, pos.ctypes.data_as(u32p), cm.ctypes.data_as(u8p),
                                           epk.ctypes.data_as(u8p), nonce.ctypes.data_as(u8p),
                                           lens.ctypes.data_as(u32p), cts.ctypes.data_as(u8p)),
              "zkmi_note_store_append")

    def append_arrays(self, positions, commitments, epks, nonces, ct_lens, cts):
        """append() over ready arrays: u32 (n), u8 (n, 32), (n, 32), (n, 12), u32 (n), u8 (sum of ct_lens)"""
        arr = [np.ascontiguousarray(a, t) for a, t in ((positions, np.uint32), (commitments, np.uint8), (epks, np.uint8),
                                                       (nonces, np.uint8), (ct_lens, np.uint32), (cts, np.uint8))]
        n = arr[0].size
        if arr[1].size != 32 * n or arr[2].size != 32 * n or arr[3].size != 12 * n or arr[4].size != n or \
                arr[5].size != int(arr[4].sum(dtype=np.uint64)):
            raise ValueError("append_arrays: array sizes do not agree")
        check(lib().zkmi_note_store_append(self.ctx.h, self.h, n, arr[0].ctypes.data_as(u32p), arr[1].ctypes.data_as(u8p),
                                           arr[2].ctypes.data_as(u8p), arr[3].ctypes.data_as(u8p),
                                           arr[4].ctypes.data_as(u32p), arr[5].ctypes.data_as(u8p)),
              "zkmi_note_store_append")

    def get(self, first: int = 0, n: int | None = None) -> list:
        """the notes [first, first + n) in append order, as append() takes them"""
        n = self.count - first if n is None else n
        m = max(n, 1)
        pos, lens = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        cm, epk, nonce = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8), np.zeros((m, 12), np.uint8)
        cts = np.zeros(m * self.max_ct, np.uint8)
        check(lib().zkmi_note_store_get(self.ctx.h, self.h, first, n, pos.ctypes.data_as(u32p), cm.ctypes.data_as(u8p),
                                        epk.ctypes.data_as(u8p), nonce.ctypes.data_as(u8p), lens.ctypes.data_as(u32p),
                                        cts.ctypes.data_as(u8p)), "zkmi_note_store_get")
        out, at = [], 0
        for i in range(n):
            out.append((int(pos[i]), cm[i].tobytes(), epk[i].tobytes(), nonce[i].tobytes(),
                        cts[at:at + int(lens[i])].tobytes()))
            at += int(lens[i])
        return out

    def scan(self, keys, owner_pks, scheme: int = COMMIT_POSEIDON, from_position: int = 0, limit: int = 1000,
             memos: bool = True):
        """zkmi_note_scan: every stored note at a position >= from_position
        against every (keys[k], owner_pks[k]) -> per key ([ScannedNote] in
        ascending position order, at most limit; scanned_to; [stats x 4]
        indexed by SCAN_*)."""
        kb, ob = _key_bytes(keys), _key_bytes(owner_pks)
        nk = kb.shape[0]
        if ob.shape[0] != nk:
            raise ValueError("scan: one owner public key per decryption key")
        if not 1 <= limit <= 65536:
            raise ValueError("scan: limit 1..65536")
        m, memo_cap = max(nk, 1), self.max_ct - 58
        counts, to, stats = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros((m, 4), np.uint32)
        pos, vals = np.zeros((m, limit), np.uint32), np.zeros((m, limit), np.uint64)
        rand, cm = np.zeros((m, limit, 32), np.uint8), np.zeros((m, limit, 32), np.uint8)
        mlen = np.zeros((m, limit), np.uint32)
        memo = np.zeros((m, limit, max(memo_cap, 1)), np.uint8) if memos else None
        kb, ob = np.ascontiguousarray(kb), np.ascontiguousarray(ob)
        check(lib().zkmi_note_scan(self.ctx.h, self.h, self.mimc.h if self.mimc is not None else None,
                                   self.poseidon.h if self.poseidon is not None else None, scheme, nk,
                                   kb.ctypes.data_as(u8p), ob.ctypes.data_as(u8p), from_position, limit,
                                   counts.ctypes.data_as(u32p), to.ctypes.data_as(u32p), stats.ctypes.data_as(u32p),
                                   pos.ctypes.data_as(u32p), _p64(vals), rand.ctypes.data_as(u8p),
                                   cm.ctypes.data_as(u8p), mlen.ctypes.data_as(u32p),
                                   None if memo is None else memo.ctypes.data_as(u8p)), "zkmi_note_scan")
        out = []
        for k in range(nk):
            hits = [ScannedNote(int(pos[k, j]), cm[k, j].tobytes(), int(vals[k, j]), rand[k, j].tobytes(),
                                memo[k, j, :int(mlen[k, j])].tobytes() if memo is not None else b"")
                    for j in range(int(counts[k]))]
            out.append((hits, int(to[k]), [int(v) for v in stats[k]]))
        return out


SIG_OK, SIG_BAD_PUBKEY, SIG_BAD_S, SIG_MISMATCH = 0, 1, 2, 3  # ZKMI_SIG_*
TX_TRANSFER, TX_WITHDRAWAL = 0, 1  # ZKMI_TX_*
TXAUTH_OK, TXAUTH_BAD_PUBKEY, TXAUTH_FAILED, TXAUTH_FROM_MISMATCH = 0, 1, 2, 3  # ZKMI_TXAUTH_*
TXFMT_NONE, TXFMT_READABLE, TXFMT_LEGACY = 0, 1, 2  # ZKMI_TXFMT_*
# zkmi_signed_tx, field for field: 192 bytes, no padding
SIGNED_TX_DTYPE = np.dtype([("from", np.uint8, 32), ("to", np.uint8, 32), ("amount", "<u8"), ("nonce", "<u8"),
                            ("chain_id", "<u8"), ("signer_pubkey", np.uint8, 32), ("signature", np.uint8, 64),
                            ("kind", np.uint8), ("reserved", np.uint8, 7)])
assert SIGNED_TX_DTYPE.itemsize == 192


class Ed25519Verifier:
    """Batched Ed25519 verification on the device (zkmi_ed25519_verify_many,
    DESIGN.md §2.16): ed25519-dalek 2.2.0 `verify` semantics, one lane per
    signature.  It holds no device state of its own: the workspace and the
    table of the base point live on the context."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def verify_many(self, pubkeys, msgs, sigs) -> np.ndarray:
        """pubkeys: n x 32 bytes, msgs: n byte strings of any length, sigs:
        n x 64 bytes -> a uint8 array of n SIG_* verdicts"""
        pubkeys, msgs, sigs = [bytes(p) for p in pubkeys], [bytes(m) for m in msgs], [bytes(s) for s in sigs]
        n = len(pubkeys)
        if len(msgs) != n or len(sigs) != n:
            raise ValueError("verify_many: one message and one signature per public key")
        if any(len(p) != 32 for p in pubkeys) or any(len(s) != 64 for s in sigs):
            raise ValueError("verify_many: 32-byte public keys and 64-byte signatures")
        off = np.zeros(n + 1, np.uint64)
        np.cumsum([len(m) for m in msgs], out=off[1:])
        return self.verify_arrays(np.frombuffer(b"".join(pubkeys), np.uint8), np.frombuffer(b"".join(sigs), np.uint8),
                                  np.frombuffer(b"".join(msgs), np.uint8), off)

    def verify_arrays(self, pubkeys, sigs, msgs, offsets) -> np.ndarray:
        """verify_many over ready arrays: u8 (n x 32), u8 (n x 64), u8 (the
        messages back to back), u64 (n + 1 offsets, [0] = 0, ascending)"""
        pk, sg, ms = (np.ascontiguousarray(a, np.uint8).reshape(-1) for a in (pubkeys, sigs, msgs))
        off = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
        n = off.size - 1
        if n < 0 or pk.size != 32 * n or sg.size != 64 * n or ms.size < int(off[-1]):
            raise ValueError("verify_arrays: array sizes do not agree")
        out = np.zeros(max(n, 1), np.uint8)
        if ms.size == 0:
            ms = np.zeros(1, np.uint8)
        check(lib().zkmi_ed25519_verify_many(self.ctx.h, n, pk.ctypes.data_as(u8p), sg.ctypes.data_as(u8p),
                                             ms.ctypes.data_as(u8p), _p64(off), out.ctypes.data_as(u8p)),
              "zkmi_ed25519_verify_many")
        return out[:n]

    def auth_records(self, records):
        """The sequencer's whole check of transfers and withdrawals from their
        fields (zkmi_tx_auth_many): the signed messages are
        built on the device, the readable format first and the legacy one for
        those it did not verify, and `from` is compared with the signer.
        records: a numpy array of SIGNED_TX_DTYPE, transfers and withdrawals
        in any mix -> (reasons, formats), two uint8 arrays of TXAUTH_* and
        TXFMT_* codes"""
        rec = np.ascontiguousarray(records)
        if rec.dtype != SIGNED_TX_DTYPE or rec.ndim != 1:
            raise ValueError("auth_records: a one-dimensional array of gpu.SIGNED_TX_DTYPE")
        n = rec.size
        reasons, formats = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        check(lib().zkmi_tx_auth_many(self.ctx.h, n, rec.ctypes.data if n else None, reasons.ctypes.data_as(u8p),
                                      formats.ctypes.data_as(u8p)), "zkmi_tx_auth_many")
        return reasons[:n], formats[:n]
