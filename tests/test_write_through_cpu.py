"""CPU: argument checks and host arithmetic of the write-through cache build
(adl_bloom_filter_cache_build / _build_device / _publish / _abandon,
adl_bloom_verify).  No device call is reached by any of these."""
import ctypes

import numpy as np


def _args():
    kb = (ctypes.c_uint64 * 2)(0, 4)
    keys = ctypes.create_string_buffer(64)
    block = ctypes.create_string_buffer(256)
    return kb, keys, block


def test_build_rejects_null_cache():
    import adlbloom

    L = adlbloom.lib()
    kb, keys, block = _args()
    t = ctypes.c_void_p()
    assert L.adl_bloom_filter_cache_build(None, ctypes.addressof(keys), None, 16, kb, 1, 10, 0,
                                          ctypes.addressof(block), 256, ctypes.byref(t), None) == -1
    assert L.adl_bloom_filter_cache_build_device(None, ctypes.addressof(keys), None, 16, kb, 1, 10, 0,
                                                 ctypes.addressof(keys), 64, ctypes.addressof(block), 256,
                                                 ctypes.byref(t), None) == -1
    assert not t.value


def test_publish_and_abandon_reject_null():
    import adlbloom

    L = adlbloom.lib()
    fake = ctypes.create_string_buffer(4096)  # never looked into: the NULL partner is checked first
    p = ctypes.addressof(fake)
    assert L.adl_bloom_filter_cache_publish(None, p, b"oid", 3) == -1
    assert L.adl_bloom_filter_cache_publish(p, None, b"oid", 3) == -1
    assert L.adl_bloom_filter_cache_abandon(None, p) == -1
    assert L.adl_bloom_filter_cache_abandon(p, None) == -1


def test_build_rejects_unknown_flags():
    """Flag bits are checked before anything else is looked at (the cache
    pointer here is a dummy the call must not touch)."""
    import adlbloom

    L = adlbloom.lib()
    kb, keys, block = _args()
    fake = ctypes.create_string_buffer(4096)
    t = ctypes.c_void_p()
    assert L.adl_bloom_filter_cache_build(ctypes.addressof(fake), ctypes.addressof(keys), None, 16, kb, 1, 10, 0x80,
                                          ctypes.addressof(block), 256, ctypes.byref(t), None) == -1
    assert L.adl_bloom_filter_cache_build_device(ctypes.addressof(fake), ctypes.addressof(keys), None, 16, kb, 1, 10,
                                                 0x80, ctypes.addressof(keys), 64, ctypes.addressof(block), 256,
                                                 ctypes.byref(t), None) == -1
    assert adlbloom.CACHE_VERIFY == 2 and adlbloom.TEST_FAULT_CACHE_BUILD_CORRUPT == 3


def test_build_workspace_bytes():
    import adlbloom

    L = adlbloom.lib()

    def ws(kb, bpk=10):
        kb = np.ascontiguousarray(kb, dtype=np.uint64)
        return (L.adl_bloom_filter_cache_build_workspace_bytes(kb.ctypes.data, len(kb) - 1, bpk),
                L.adl_bloom_filter_block_workspace_bytes(kb.ctypes.data, len(kb) - 1, bpk))

    assert ws([0, 10, 5])[0] == 0  # decreasing key_begin
    # a block beyond the reference's int offsets (test_filter_block_bytes_matches_oracle_framing's case)
    kb = np.arange(10, dtype=np.uint64) * 26_000_000
    assert ws(kb)[0] == 0
    assert ws(kb[:8])[0] > 0
    for shape in ([0, 0], [0, 1], [0, 120_001], [0, 0, 1, 3001, 3001, 123_002], [0, 1, 778, 40_778]):
        for bpk in (0, 3, 10, 16, 44):
            mine, base = ws(shape, bpk)
            assert base > 0 and mine >= base, (shape, bpk)
    assert ws([0, 5], -1)[0] == 0
    assert L.adl_bloom_filter_cache_build_workspace_bytes(None, 1, 10) == 0


def test_verify_argument_checks():
    """adl_bloom_verify with nothing to check answers (0, ~0) without a device call."""
    import adlbloom

    L = adlbloom.lib()
    m, f = ctypes.c_uint64(7), ctypes.c_uint64(7)
    kb = (ctypes.c_uint64 * 2)(0, 0)
    assert L.adl_bloom_verify(None, None, 0, 16, kb, 1, None, kb, 10, ctypes.byref(m), ctypes.byref(f), None) == 0
    assert m.value == 0 and f.value == 2**64 - 1
    assert L.adl_bloom_verify(None, None, 0, 16, kb, 1, None, kb, 10, None, ctypes.byref(f), None) == -1
    assert L.adl_bloom_verify(None, None, 4, 16, kb, 1, None, kb, 10, ctypes.byref(m), ctypes.byref(f), None) == -1
    assert L.adl_bloom_verify_device(None, None, 0, 16, None, 0, None, None, None, 10, None, None) == -1
