"""CPU: the fan-out probe's C-ABI surface (adl_bloom_probe_fanout_device,
adl_bloom_filter_cache_probe_fanout) -- declared, exported, argument checks
made before any device call -- and its kernels in the built gfx950 code object
(all three key views, no scratch).  No compute call is made here."""
import ctypes
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adl_bloom.h")
LIB = os.path.join(ROOT, "adlsm-tree_amd", "lib", "libadlbloom.so")
NEW = ("adl_bloom_probe_fanout_device", "adl_bloom_filter_cache_probe_fanout")
INVALID_ARG = -1


def test_symbols_declared_and_exported():
    import adlbloom

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = adlbloom.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in adlbloom.EXPORTS
        assert hasattr(L, name), name
    assert L.adl_bloom_abi_version() == 1  # additive: the version stays


def test_cache_probe_fanout_null_cache():
    import adlbloom

    L = adlbloom.lib()
    key = ctypes.create_string_buffer(16)
    pb = (ctypes.c_uint32 * 2)(0, 1)
    pt = (ctypes.c_uint32 * 1)(0)
    out = ctypes.create_string_buffer(1)
    unc = ctypes.c_uint64(7)
    rc = L.adl_bloom_filter_cache_probe_fanout(None, None, None, 0, 0, ctypes.addressof(key), None, 1, 16,
                                               ctypes.addressof(pb), ctypes.addressof(pt), ctypes.addressof(out),
                                               ctypes.byref(unc), None)
    assert rc == INVALID_ARG


def test_probe_fanout_device_no_keys_is_ok():
    import adlbloom

    L = adlbloom.lib()
    assert L.adl_bloom_probe_fanout_device(None, None, 0, 16, None, None, 0, 0, None, None, None, 10, None,
                                           None) == adlbloom.ADL_OK
    # keys but no pairs: nothing to answer either
    buf = ctypes.create_string_buffer(64)
    assert L.adl_bloom_probe_fanout_device(ctypes.addressof(buf), None, 2, 16, ctypes.addressof(buf), None, 0, 0,
                                           None, None, None, 10, None, None) == adlbloom.ADL_OK


def test_probe_fanout_device_rejects_null_out():
    """The pointers here are host addresses that are never dereferenced: the
    argument check returns before any launch."""
    import adlbloom

    L = adlbloom.lib()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    assert L.adl_bloom_probe_fanout_device(a, None, 2, 16, a, a, 3, 1, a, a, None, 10, None, None) == INVALID_ARG
    # the other rules of adl_bloom_probe_ranges_device: bits_per_key, stride, the filter tables
    assert L.adl_bloom_probe_fanout_device(a, None, 2, 16, a, a, 3, 1, a, a, None, -1, a, None) == INVALID_ARG
    assert L.adl_bloom_probe_fanout_device(a, None, 2, 0, a, a, 3, 1, a, a, None, 10, a, None) == INVALID_ARG
    assert L.adl_bloom_probe_fanout_device(a, None, 2, 16, a, a, 3, 1, None, a, None, 10, a, None) == INVALID_ARG
    assert L.adl_bloom_probe_fanout_device(a, None, 2, 16, a, None, 3, 1, a, a, None, 10, a, None) == INVALID_ARG


@pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which("llvm-readelf", path="/opt/rocm/lib/llvm/bin")),
                    reason="needs the built library and ROCm's llvm tools")
def test_fanout_kernels_in_code_object_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    res = kernel_resources.kernel_resources(LIB)
    for view in ("Keys16", "KeysStride", "KeysVar"):
        mine = {k: r for k, r in res.items() if "bloom_probe_fanout_kernel" in k and view in k}
        assert len(mine) == 1, (view, sorted(mine))
        (r,) = mine.values()
        assert r["scratch"] == 0, (view, r)
