"""Every entry point that takes a context refuses a null one with LSMBLK_E_INVAL (CPU only).

The entry points validate their arguments before they take the context's lock (CallGuard,
lsmblk_dev.hpp, dereferences the context), so a null context with every other argument zero or
null must come back as LSMBLK_E_INVAL from each of them, without touching a device.  A new entry
point has to be classified here: the test counts the functions it called."""
import ctypes

from lsm_amd import _lib

# symbols of include/lsmblk.h that take no lsmblk_ctx
NO_CTX_FAMILIES = ("lsmblk_builder_", "lsmblk_block_", "lsmblk_iter_", "lsmblk_memtable_")
NO_CTX = {"lsmblk_abi_version", "lsmblk_strerror", "lsmblk_stats_status", "lsmblk_ctx_create", "lsmblk_ctx_destroy",
          "lsmblk_shard_halo_entries", "lsmblk_fingerprint32", "lsmblk_bloom_may_contain"}
CTX_ENTRY_POINTS = 31


def takes_ctx(name):
    if name == "lsmblk_block_meta_batch":
        return True
    return name not in NO_CTX and not name.startswith(NO_CTX_FAMILIES)


def zero_of(t):
    if t in (_lib.P, _lib.PP) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return None
    return t(0)


def test_null_context_is_invalid_everywhere():
    L = _lib.lib()
    called = []
    for name, res, args in _lib.SIGNATURES:
        if not takes_ctx(name):
            continue
        assert res is _lib.I and args and args[0] is _lib.P, name
        rc = getattr(L, name)(*[zero_of(t) for t in args])
        assert rc == _lib.LSMBLK_E_INVAL, (name, rc)
        called.append(name)
    assert len(called) == CTX_ENTRY_POINTS, sorted(called)
