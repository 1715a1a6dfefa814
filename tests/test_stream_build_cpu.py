"""CPU: the streamed build's C-ABI (adl_bloom_stream_*) without a device:
argument refusals that return before any device call, the host-side filter
bounds, the finish workspace size, and the append kernels in the code object.
An adl_bloom_stream allocates nothing before its first append, so creating,
cutting and sizing one needs no GPU."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -2


@pytest.fixture
def L():
    import adlbloom

    return adlbloom.lib()


@pytest.fixture
def stream(L):
    h = ctypes.c_void_p()
    assert L.adl_bloom_stream_create(1000, ctypes.byref(h)) == 0 and h.value
    yield h
    assert L.adl_bloom_stream_destroy(h) == 0


def test_null_object_is_refused(L):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    off = (ctypes.c_uint64 * 1)(0)
    nf = ctypes.c_uint32()
    assert L.adl_bloom_stream_create(0, None) == INVALID
    assert L.adl_bloom_stream_destroy(None) == INVALID
    assert L.adl_bloom_stream_reset(None) == INVALID
    assert L.adl_bloom_stream_cut(None) == INVALID
    assert L.adl_bloom_stream_append(None, p, None, 1, 16, None) == INVALID
    assert L.adl_bloom_stream_append_device(None, p, None, 1, 16, None) == INVALID
    assert L.adl_bloom_stream_counts(None, ctypes.byref(nf), None, 0) == INVALID
    assert L.adl_bloom_stream_finish_workspace_bytes(None, 10) == 0
    assert L.adl_bloom_stream_finish_device(None, 10, 0, p, off, p, 64, None) == INVALID
    assert L.adl_bloom_stream_finish(None, 10, 0, p, off, None) == INVALID
    got, t = ctypes.c_uint64(), ctypes.c_void_p()
    # (a cache needs a device; without one and without a stream the call is refused first)
    assert L.adl_bloom_filter_cache_build_stream(None, None, 10, 0, p, 64, ctypes.byref(got), ctypes.byref(t), None) == INVALID
    assert L.adl_bloom_filter_cache_build_stream(None, None, 10, 0x80, p, 64, ctypes.byref(got), ctypes.byref(t), None) == INVALID


def test_append_refusals(L, stream):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for fn in (L.adl_bloom_stream_append, L.adl_bloom_stream_append_device):
        assert fn(stream, None, None, 3, 16, None) == INVALID   # NULL keys with n > 0
        assert fn(stream, p, None, 3, 0, None) == INVALID       # stride 0 without offsets
        assert fn(stream, p, None, 2**31, 16, None) == TOO_LARGE
        assert fn(stream, None, None, 0, 0, None) == 0          # n == 0: a no-op
    offs = (ctypes.c_uint64 * 4)(0, 8, 4, 12)                   # decreasing host offsets
    assert L.adl_bloom_stream_append(stream, p, offs, 3, 0, None) == INVALID
    nf = ctypes.c_uint32(99)
    assert L.adl_bloom_stream_counts(stream, ctypes.byref(nf), None, 0) == 0 and nf.value == 0


def test_finish_refusals(L, stream):
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    off = (ctypes.c_uint64 * 2)(0, 16)
    # no filter yet
    assert L.adl_bloom_stream_finish_device(stream, 10, 0, p, off, p, 64, None) == INVALID
    assert L.adl_bloom_stream_cut(stream) == 0
    assert L.adl_bloom_stream_cut(stream) == 0
    for fd in (lambda bpk, flags, out, o: L.adl_bloom_stream_finish_device(stream, bpk, flags, out, o, p, 64, None),
               lambda bpk, flags, out, o: L.adl_bloom_stream_finish(stream, bpk, flags, out, o, None)):
        assert fd(-1, 0, p, off) == INVALID      # negative bits_per_key
        assert fd(10, 0x80, p, off) == INVALID   # unknown flags
        assert fd(10, 2, p, off) == INVALID      # (ADL_BLOOM_CACHE_VERIFY is no build flag)
        assert fd(10, 0, None, off) == INVALID
        assert fd(10, 0, p, None) == INVALID
    assert L.adl_bloom_stream_finish_device(stream, 10, 0, p + 8, off, p, 64, None) == INVALID   # bitmaps not 16-byte aligned
    bad = (ctypes.c_uint64 * 2)(0, 8)
    assert L.adl_bloom_stream_finish_device(stream, 10, 0, p, bad, p, 64, None) == INVALID
    assert L.adl_bloom_stream_finish_device(stream, 10, 0, p, off, None, 0, None) == -5  # ADL_ERR_WORKSPACE


def test_counts_and_workspace_of_a_cut_only_object(L, stream):
    import adlbloom

    nf = ctypes.c_uint32()
    for want in (1, 2, 3):
        assert L.adl_bloom_stream_cut(stream) == 0
        assert L.adl_bloom_stream_counts(stream, ctypes.byref(nf), None, 0) == 0 and nf.value == want
    kb = np.full(4, 7, dtype=np.uint64)
    assert L.adl_bloom_stream_counts(stream, ctypes.byref(nf), kb.ctypes.data, 3) == INVALID and nf.value == 3
    assert L.adl_bloom_stream_counts(stream, ctypes.byref(nf), kb.ctypes.data, 4) == 0
    assert list(kb) == [0, 0, 0, 0]
    for bpk in (0, 3, 10, 44):
        ws = L.adl_bloom_stream_finish_workspace_bytes(stream, bpk)
        assert ws == adlbloom.workspace_bytes([0, 0, 0], bpk) and ws > 0
    assert L.adl_bloom_stream_finish_workspace_bytes(stream, -1) == 0
    assert L.adl_bloom_stream_reset(stream) == 0
    assert L.adl_bloom_stream_counts(stream, ctypes.byref(nf), None, 0) == 0 and nf.value == 0
    assert L.adl_bloom_stream_finish_workspace_bytes(stream, 10) == 0


def test_python_wrapper_bounds():
    import adlbloom

    sb = adlbloom.StreamBuilder(reserve_keys=10)
    assert list(sb.counts()) == [0]
    sb.cut()
    sb.cut()
    assert list(sb.counts()) == [0, 0, 0]
    assert sb.workspace_bytes(10) == adlbloom.workspace_bytes([0, 0], 10)
    assert adlbloom.STREAM_RUN_KEYS == 512
    sb.reset()
    assert list(sb.counts()) == [0]
    sb.close()
    sb.close()


@pytest.mark.skipif(not shutil.which("llvm-readelf", path="/opt/rocm/lib/llvm/bin"), reason="needs ROCm's llvm tools")
def test_append_kernels_in_the_code_object():
    import adlbloom

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    res = kernel_resources.kernel_resources(adlbloom.LIB_PATH)
    for frag in ("hash16_pairs_kernel", "hash_run_pairs_kernel", "bloom_bin16_kernelILi1024ELi6ENS_4SrcP",
                 "8KeysPair"):
        found = {k: r for k, r in res.items() if frag in k}
        assert found, frag
        for k, r in found.items():
            assert r["scratch"] == 0, (k, r)
            if "bloom_bin" in k:
                assert r["vgpr"] <= 120, (k, r)
    runs = [k for k in res if "hash_run_pairs_kernel" in k]
    assert len(runs) == 4  # var-len and fixed stride, whole-block and exact reads
