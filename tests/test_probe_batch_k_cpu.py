"""CPU: the large-batch probe with a probe count per filter -- its four C-ABI
symbols and adl_bloom_probe_batch_k_workspace_bytes.

The plan of a call with a k per filter is made from max_k, the bound on every
filter's k: its size is the uniform plan's for a bits_per_key whose k is max_k,
it does not shrink as max_k grows, a batch the pipeline does not take needs 256
bytes, and max_k outside 1..30 gives 0.  ADL_BLOOM_PROBE_BATCH_MAX_K keeps
batches whose max_k is above it on the direct kernel (256 bytes), so the sizes
are taken with the knob at 30, no limit.  Needs the built library,
no GPU.
"""
import ctypes
import itertools

import pytest

VAR_MIN = "ADL_BLOOM_PROBE_BATCH_VAR_MIN"
MAX_K = "ADL_BLOOM_PROBE_BATCH_MAX_K"
NS = [(1 << 20) - 1, 1 << 20, (1 << 20) + 777, 1 << 24]
FS = [1, 7, 4096, 4097]
STRIDES = [16, 0, 24]
GRID = list(itertools.product(NS, FS, STRIDES))
BPKS = [1, 2, 3, 5, 10, 11, 16, 20, 30, 43, 44, 100]  # k = 1, 1, 2, 3, 6, 7, 11, 13, 20, 29, 30, 30


@pytest.fixture(scope="module")
def L():
    import adlbloom

    return adlbloom.lib()


def takes_pipeline(n, f, stride, var_min):
    """include/adl_bloom.h: 16-byte keys from 2^20 queries on, other shapes from the knob (0: never)."""
    if not (1 <= f <= 4096 and n < (1 << 31) - 1):
        return False
    return n >= (1 << 20) if stride == 16 else bool(var_min) and n >= max(var_min, 1 << 20)


def test_symbols_and_argument_types(L):
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    chars = ctypes.POINTER(ctypes.c_char_p)
    want = {
        "adl_bloom_probe_batch_k_workspace_bytes": (u64, [u64, u32, u32, u32]),
        "adl_bloom_probe_batch_k_device": (ctypes.c_int, [vp, vp, u64, u32, vp, u32, vp, vp, vp, vp, u32, vp, vp, u64,
                                                           vp]),
        "adl_bloom_filter_cache_probe_batch_workspace_bytes": (u64, [vp, chars, vp, u32, u64, u32]),
        "adl_bloom_filter_cache_probe_batch_device": (ctypes.c_int, [vp, chars, vp, u32, u32, vp, vp, u64, u32, vp, vp,
                                                                      vp, vp, u64, vp]),
    }
    for name, (res, args) in want.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_python_wrappers_exist():
    import adlbloom

    assert callable(adlbloom.probe_batch_k)
    assert callable(adlbloom.FilterCache.probe_batch_device)
    assert callable(adlbloom.FilterCache.probe_batch_workspace_bytes)


@pytest.mark.parametrize("var_min", [0, 1])
def test_equals_the_uniform_size_at_max_k_of_bpk(L, knobs, var_min):
    knobs.set(VAR_MIN, var_min)
    knobs.set(MAX_K, 30)  # no limit: the sizes of every max_k
    for n, f, stride in GRID:
        for bpk in BPKS:
            k = L.adl_bloom_num_probes(bpk)
            assert (L.adl_bloom_probe_batch_k_workspace_bytes(n, f, k, stride) ==
                    L.adl_bloom_probe_batch_workspace_bytes(n, f, bpk, stride)), (n, f, stride, bpk)


@pytest.mark.parametrize("var_min", [0, 1])
def test_non_decreasing_in_max_k(L, knobs, var_min):
    """The chunk size C = (38844 / k) & ~63 is quantised, so a single plan is not
    monotone in k where the F + 1 spare chunks dominate (4096 filters, 2^20
    queries: the plan of k = 12 is smaller than that of 11).  The size functions
    promise the largest plan of any k' <= k, so a workspace sized for max_k
    serves every call with a smaller one."""
    knobs.set(VAR_MIN, var_min)
    knobs.set(MAX_K, 30)  # no limit: the sizes of every max_k
    for n, f, stride in GRID:
        sizes = [L.adl_bloom_probe_batch_k_workspace_bytes(n, f, k, stride) for k in range(1, 31)]
        assert sizes == sorted(sizes), (n, f, stride, sizes)
        if takes_pipeline(n, f, stride, var_min):
            assert sizes[0] > 256 and sizes[-1] > sizes[0], (n, f, stride)


@pytest.mark.parametrize("var_min", [0, 1])
def test_256_for_direct_batches_and_0_for_a_max_k_out_of_range(L, knobs, var_min):
    knobs.set(VAR_MIN, var_min)
    knobs.set(MAX_K, 30)  # no limit: the sizes of every max_k
    for n, f, stride in GRID:
        for k in (1, 6, 30):
            got = L.adl_bloom_probe_batch_k_workspace_bytes(n, f, k, stride)
            assert (got > 256) if takes_pipeline(n, f, stride, var_min) else (got == 256), (n, f, stride, k)
        for k in (0, 31, 255, 1 << 31):
            assert L.adl_bloom_probe_batch_k_workspace_bytes(n, f, k, stride) == 0, (n, f, stride, k)
    assert L.adl_bloom_probe_batch_k_workspace_bytes((1 << 31) - 2, 7, 6, 16) > 256
    assert L.adl_bloom_probe_batch_k_workspace_bytes((1 << 31) - 1, 7, 6, 16) == 256
    assert L.adl_bloom_probe_batch_k_workspace_bytes(1 << 20, 0, 6, 16) == 256


def test_max_k_knob_turns_a_batch_direct(L, knobs):
    knobs.set(VAR_MIN, 1)
    n, f = (1 << 20) + 777, 7
    knobs.set(MAX_K, 30)
    for stride in STRIDES:
        assert all(L.adl_bloom_probe_batch_k_workspace_bytes(n, f, k, stride) > 256 for k in range(1, 31))
    knobs.set(MAX_K, 7)
    for stride in STRIDES:
        assert all(L.adl_bloom_probe_batch_k_workspace_bytes(n, f, k, stride) > 256 for k in range(1, 8))
        assert all(L.adl_bloom_probe_batch_k_workspace_bytes(n, f, k, stride) == 256 for k in range(8, 31))
        assert L.adl_bloom_probe_batch_k_workspace_bytes(n, f, 31, stride) == 0
    knobs.set(MAX_K, 0)
    assert L.adl_bloom_probe_batch_k_workspace_bytes(n, f, 1, 16) == 256
    knobs.unset(MAX_K)  # the default: 2, the measured crossover at 2^24 queries
    assert L.adl_bloom_probe_batch_k_workspace_bytes(n, f, 2, 16) > 256
    assert L.adl_bloom_probe_batch_k_workspace_bytes(n, f, 3, 16) == 256
    # the knob is not about the uniform entry point
    assert L.adl_bloom_probe_batch_workspace_bytes(n, f, 44, 16) > 256
