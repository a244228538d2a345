"""zelana_amd — MI355X-native BN254 Groth16 proving backend for Zelana's L2
batch-proof path.  The compute lives in libzkmi.so (HIP for
gfx950, C ABI in include/zkmi.h); this package is the host-side mirror of the
reference's BatchProver interface plus ctypes plumbing."""

# names of zelana_amd/shielded.py and shielded_pool.py handed out on first use
_SHIELDED = ("ShieldedProver", "DeviceNoteTree", "shielded_hasher", "commit_many", "nullifier_many",
             "derive_pk_many", "honest_many")
_POOL = ("ShieldedPool",)
__all__ = ["ZkmiError", *_SHIELDED, *_POOL]

from ._lib import ZkmiError  # noqa: E402


def __getattr__(name):
    # on first use: the package import stays as light as it was (no
    # numpy-heavy module, no library load)
    if name in _SHIELDED:
        from . import shielded
        return getattr(shielded, name)
    if name in _POOL:
        from . import shielded_pool
        return getattr(shielded_pool, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
