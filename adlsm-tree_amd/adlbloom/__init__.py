"""adlbloom -- Python binding of libadlbloom.so (include/adl_bloom.h) over ctypes.

The product path: every build/probe here runs the gfx950 HIP kernels through
the C-ABI.  There is no CPU fallback -- if the shared library or a GPU is
missing, the calls raise.  torch is used only for device memory and streams.

Reference interfaces mirrored (adlternative/adlsm-tree):
  * build()  ~ BloomFilter::Keys2Block          src/filter_block.cpp:9-33
  * probe()  ~ BloomFilter::IsKeyExists         src/filter_block.cpp:49-62
  * murmur3  ~ murmur3_hash                     src/murmur3_hash.cpp:11-65
  * num_probes / bitmap_bytes                   src/filter_block.cpp:11-14, 44-46
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ADL_BLOOM_LIB: diagnostics only (tools/stamps.py points it at the
# s_memtime-instrumented build, lib_stamps/libadlbloom.so)
LIB_PATH = os.environ.get("ADL_BLOOM_LIB") or os.path.join(PKG_DIR, "lib", "libadlbloom.so")

SEED1 = 0xE2C6928A  # src/filter_block.cpp:22
SEED2 = 0xBAEA8A8F  # src/filter_block.cpp:23

ADL_OK = 0
ADL_FILTER_BLOCK_ERROR = 13

# every symbol include/adl_bloom.h declares (tests check the .so exports them all)
EXPORTS = (
    "adl_bloom_strerror", "adl_bloom_abi_version", "adl_bloom_num_probes",
    "adl_bloom_bitmap_bytes", "adl_bloom_bitmap_alloc_bytes", "adl_bloom_build_workspace_bytes",
    "adl_bloom_build_device", "adl_bloom_build_segmented_device", "adl_bloom_build",
    "adl_bloom_build_segmented", "adl_bloom_filter_block_bytes", "adl_bloom_filter_block_workspace_bytes",
    "adl_bloom_filter_block_build_device", "adl_bloom_probe_ranges_device", "adl_bloom_build_segmented_device_ex",
    "adl_bloom_filter_cache_create", "adl_bloom_filter_cache_destroy", "adl_bloom_filter_cache_put",
    "adl_bloom_filter_cache_contains", "adl_bloom_filter_cache_remove", "adl_bloom_filter_cache_stats",
    "adl_bloom_filter_cache_probe",
    "adl_bloom_probe_device", "adl_bloom_probe_multi_device", "adl_bloom_probe",
    "adl_bloom_filter_set_create", "adl_bloom_filter_set_probe",
    "adl_bloom_filter_set_device_view", "adl_bloom_filter_set_destroy",
    "adl_bloom_murmur3_device", "adl_bloom_murmur3", "adl_synth_keys16_device",
    "adl_synth_varlen_lengths_device", "adl_synth_varlen_fill_device",
    "adl_bloom_profile_enable", "adl_bloom_profile_collect", "adl_synth_probe_queries_device",
    "adl_bloom_profile_each", "adl_bloom_probe_batch_workspace_bytes", "adl_bloom_probe_batch_device",
    "adl_bloom_test_fault", "adl_bloom_build_positions", "adl_bloom_get_device", "adl_bloom_set_device",
    "adl_bloom_reload_knobs", "adl_bloom_build_segmented_ex", "adl_bloom_probe_server_launches",
    "adl_bloom_probe_server_phases", "adl_bloom_probe_fanout_device", "adl_bloom_filter_cache_probe_fanout",
    "adl_bloom_filter_cache_build", "adl_bloom_filter_cache_build_workspace_bytes",
    "adl_bloom_filter_cache_build_device", "adl_bloom_filter_cache_publish", "adl_bloom_filter_cache_abandon",
    "adl_bloom_verify_device", "adl_bloom_verify",
    "adl_bloom_level_create", "adl_bloom_level_destroy", "adl_bloom_level_stats",
    "adl_bloom_level_candidates_workspace_bytes",
    "adl_bloom_level_candidates_device", "adl_bloom_level_multiget",
    "adl_bloom_revision_create", "adl_bloom_revision_destroy", "adl_bloom_revision_stats",
    "adl_bloom_revision_candidates_workspace_bytes", "adl_bloom_revision_candidates_device",
    "adl_bloom_probe_fanout_hits_workspace_bytes", "adl_bloom_probe_fanout_hits_device",
    "adl_bloom_revision_multiget",
    "adl_bloom_hits_by_table_workspace_bytes", "adl_bloom_hits_by_table_device", "adl_bloom_revision_read_plan",
    "adl_bloom_filter_cache_probe_key", "adl_bloom_revision_candidates_host", "adl_bloom_revision_get",
    "adl_bloom_probe_batch_k_workspace_bytes", "adl_bloom_probe_batch_k_device",
    "adl_bloom_filter_cache_probe_batch_workspace_bytes", "adl_bloom_filter_cache_probe_batch_device",
    "adl_bloom_stream_create", "adl_bloom_stream_destroy", "adl_bloom_stream_reset", "adl_bloom_stream_append",
    "adl_bloom_stream_append_device", "adl_bloom_stream_cut", "adl_bloom_stream_counts",
    "adl_bloom_stream_finish_workspace_bytes", "adl_bloom_stream_finish_device", "adl_bloom_stream_finish",
    "adl_bloom_filter_cache_build_stream",
)

# keys per workgroup of the streamed build's append kernel for keys that are not aligned 16-byte keys
# (include/adl_bloom.h: ADL_BLOOM_STREAM_RUN_KEYS)
STREAM_RUN_KEYS = 512

# one resident-server request holds a single-key Get of up to this many tables and key bytes
# (include/adl_bloom.h: ADL_BLOOM_GET_MAX_TABLES, ADL_BLOOM_GET_MAX_KEY_BYTES)
GET_MAX_TABLES = 24
GET_MAX_KEY_BYTES = 96

# entries per workgroup of the grouping kernels (csrc/read_plan.hip, kTile): a tile of the radix sort
HITS_TILE = 2048

_LIB = None


class AdlBloomError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = lib().adl_bloom_strerror(status).decode()
        super().__init__(f"{what}: {msg} (status {status})" if what else f"{msg} (status {status})")


def lib() -> ctypes.CDLL:
    """Load libadlbloom.so (raises if it has not been built -- no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C adlsm-tree_amd)")
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    sig = {
        "adl_bloom_strerror": (ctypes.c_char_p, [ctypes.c_int]),
        "adl_bloom_abi_version": (ctypes.c_int, []),
        "adl_bloom_num_probes": (i32, [i32]),
        "adl_bloom_bitmap_bytes": (u64, [u64, i32]),
        "adl_bloom_bitmap_alloc_bytes": (u64, [u64, i32]),
        "adl_bloom_build_workspace_bytes": (u64, [vp, u32, i32]),
        "adl_bloom_build_device": (ctypes.c_int, [vp, vp, u64, u32, i32, vp, vp, u64, vp]),
        "adl_bloom_build_segmented_device": (ctypes.c_int, [vp, vp, u32, vp, u32, i32, vp, vp, vp, u64, vp]),
        "adl_bloom_build": (ctypes.c_int, [vp, vp, u64, u32, i32, vp, vp]),
        "adl_bloom_build_segmented": (ctypes.c_int, [vp, vp, u32, vp, u32, i32, vp, vp, vp]),
        "adl_bloom_build_segmented_ex": (ctypes.c_int, [vp, vp, u32, vp, u32, i32, vp, vp, u32, vp]),
        "adl_bloom_filter_block_bytes": (u64, [vp, u32, i32]),
        "adl_bloom_filter_block_workspace_bytes": (u64, [vp, u32, i32]),
        "adl_bloom_filter_block_build_device": (ctypes.c_int, [vp, vp, u32, vp, u32, i32, vp, u64, vp, u64, vp]),
        "adl_bloom_build_segmented_device_ex": (ctypes.c_int, [vp, vp, u32, vp, u32, i32, vp, vp, u32, vp, u64, vp]),
        "adl_bloom_probe_ranges_device": (ctypes.c_int, [vp, vp, u64, u32, vp, u32, vp, vp, vp, i32, vp, vp]),
        "adl_bloom_filter_cache_create": (ctypes.c_int, [u64, u32, i32, ctypes.POINTER(vp)]),
        "adl_bloom_filter_cache_destroy": (ctypes.c_int, [vp]),
        "adl_bloom_filter_cache_put": (ctypes.c_int, [vp, ctypes.c_char_p, u64, vp, u64]),
        "adl_bloom_filter_cache_contains": (ctypes.c_int, [vp, ctypes.c_char_p, u64]),
        "adl_bloom_filter_cache_remove": (ctypes.c_int, [vp, ctypes.c_char_p, u64]),
        "adl_bloom_filter_cache_stats": (ctypes.c_int, [vp, ctypes.POINTER(u32), ctypes.POINTER(u64)]),
        "adl_bloom_filter_cache_probe": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_char_p), vp, u32, u32, vp, vp,
                                                         u64, u32, vp, vp, ctypes.POINTER(u64), vp]),
        "adl_bloom_filter_cache_probe_fanout": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_char_p), vp, u32, u32, vp,
                                                                vp, u64, u32, vp, vp, vp, ctypes.POINTER(u64), vp]),
        "adl_bloom_probe_fanout_device": (ctypes.c_int, [vp, vp, u64, u32, vp, vp, u64, u32, vp, vp, vp, i32, vp, vp]),
        "adl_bloom_filter_cache_build": (ctypes.c_int, [vp, vp, vp, u32, vp, u32, i32, u32, vp, u64,
                                                         ctypes.POINTER(vp), vp]),
        "adl_bloom_filter_cache_build_workspace_bytes": (u64, [vp, u32, i32]),
        "adl_bloom_filter_cache_build_device": (ctypes.c_int, [vp, vp, vp, u32, vp, u32, i32, u32, vp, u64, vp, u64,
                                                                ctypes.POINTER(vp), vp]),
        "adl_bloom_filter_cache_publish": (ctypes.c_int, [vp, vp, ctypes.c_char_p, u64]),
        "adl_bloom_filter_cache_abandon": (ctypes.c_int, [vp, vp]),
        "adl_bloom_verify_device": (ctypes.c_int, [vp, vp, u64, u32, vp, u32, vp, vp, vp, i32, vp, vp]),
        "adl_bloom_verify": (ctypes.c_int, [vp, vp, u64, u32, vp, u32, vp, vp, i32, ctypes.POINTER(u64),
                                             ctypes.POINTER(u64), vp]),
        "adl_bloom_level_create": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, u32, u64, ctypes.POINTER(vp)]),
        "adl_bloom_level_destroy": (ctypes.c_int, [vp]),
        "adl_bloom_level_stats": (ctypes.c_int, [vp, ctypes.POINTER(u32), ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                  ctypes.POINTER(u32)]),
        "adl_bloom_level_candidates_workspace_bytes": (u64, [u64]),
        "adl_bloom_level_candidates_device": (ctypes.c_int, [vp, vp, vp, u64, u32, ctypes.c_int64, vp, vp, u64, vp,
                                                              vp, u64, vp]),
        "adl_bloom_level_multiget": (ctypes.c_int, [vp, vp, u32, vp, vp, u64, u32, ctypes.c_int64, vp, vp, vp, u64,
                                                     ctypes.POINTER(u64), ctypes.POINTER(u64), vp]),
        "adl_bloom_revision_create": (ctypes.c_int, [vp, u32, ctypes.POINTER(vp)]),
        "adl_bloom_revision_destroy": (ctypes.c_int, [vp]),
        "adl_bloom_revision_stats": (ctypes.c_int, [vp, ctypes.POINTER(u32), vp, ctypes.POINTER(u32)]),
        "adl_bloom_revision_candidates_workspace_bytes": (u64, [vp, u64]),
        "adl_bloom_revision_candidates_device": (ctypes.c_int, [vp, vp, vp, u64, u32, ctypes.c_int64, vp, vp, u64, vp,
                                                                 vp, u64, vp]),
        "adl_bloom_probe_fanout_hits_workspace_bytes": (u64, [u64, u64]),
        "adl_bloom_probe_fanout_hits_device": (ctypes.c_int, [vp, vp, u64, u32, vp, vp, u64, u32, vp, vp, vp, i32, vp,
                                                               vp, u64, vp, vp, u64, vp]),
        "adl_bloom_revision_multiget": (ctypes.c_int, [vp, vp, u32, vp, vp, u64, u32, ctypes.c_int64, vp, vp, u64,
                                                        ctypes.POINTER(u64), u64, ctypes.POINTER(u64),
                                                        ctypes.POINTER(u64), vp]),
        "adl_bloom_hits_by_table_workspace_bytes": (u64, [u64, u64, u32]),
        "adl_bloom_hits_by_table_device": (ctypes.c_int, [vp, vp, u64, u32, vp, vp, u64, vp, u64, vp, vp, u64, vp]),
        "adl_bloom_revision_read_plan": (ctypes.c_int, [vp, vp, u32, vp, vp, u64, u32, ctypes.c_int64, vp, vp, u64,
                                                         ctypes.POINTER(u64), vp, u64, ctypes.POINTER(u64), u64,
                                                         ctypes.POINTER(u64), ctypes.POINTER(u64), vp]),
        "adl_bloom_filter_cache_probe_key": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_char_p), vp, u32, u32, vp, u64,
                                                             vp, ctypes.POINTER(u64), vp]),
        "adl_bloom_revision_candidates_host": (ctypes.c_int, [vp, vp, u64, ctypes.c_int64, vp, u32,
                                                               ctypes.POINTER(u32)]),
        "adl_bloom_revision_get": (ctypes.c_int, [vp, vp, u32, vp, u64, ctypes.c_int64, vp, u32, ctypes.POINTER(u32),
                                                   ctypes.POINTER(u32), ctypes.POINTER(u32), vp]),
        "adl_bloom_probe_device": (ctypes.c_int, [vp, vp, u64, u32, i32, vp, u64, vp, vp]),
        "adl_bloom_probe_batch_workspace_bytes": (u64, [u64, u32, i32, u32]),
        "adl_bloom_probe_batch_device": (ctypes.c_int, [vp, vp, u64, u32, vp, u32, vp, vp, vp, i32, vp, vp, u64, vp]),
        "adl_bloom_probe_batch_k_workspace_bytes": (u64, [u64, u32, u32, u32]),
        "adl_bloom_probe_batch_k_device": (ctypes.c_int, [vp, vp, u64, u32, vp, u32, vp, vp, vp, vp, u32, vp, vp, u64,
                                                           vp]),
        "adl_bloom_filter_cache_probe_batch_workspace_bytes": (u64, [vp, ctypes.POINTER(ctypes.c_char_p), vp, u32, u64,
                                                                     u32]),
        "adl_bloom_filter_cache_probe_batch_device": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_char_p), vp, u32, u32,
                                                                      vp, vp, u64, u32, vp, vp, vp, vp, u64, vp]),
        "adl_bloom_probe_multi_device": (ctypes.c_int, [vp, vp, u64, u32, vp, u32, vp, vp, i32, vp, vp]),
        "adl_bloom_probe": (ctypes.c_int, [vp, vp, u64, u32, i32, vp, u64, vp, vp]),
        "adl_bloom_filter_set_create": (ctypes.c_int, [vp, vp, u32, i32, ctypes.POINTER(vp)]),
        "adl_bloom_filter_set_probe": (ctypes.c_int, [vp, vp, vp, u64, u32, vp, u32, vp, vp]),
        "adl_bloom_filter_set_device_view": (ctypes.c_int, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                                            ctypes.POINTER(u32)]),
        "adl_bloom_filter_set_destroy": (ctypes.c_int, [vp]),
        "adl_bloom_murmur3_device": (ctypes.c_int, [vp, vp, u64, u32, u32, u32, vp, vp]),
        "adl_bloom_murmur3": (ctypes.c_int, [u32, vp, u64, ctypes.POINTER(u32)]),
        "adl_synth_keys16_device": (ctypes.c_int, [vp, u64, u64, u64, vp]),
        "adl_synth_varlen_lengths_device": (ctypes.c_int, [vp, u64, u64, ctypes.c_double, vp]),
        "adl_synth_varlen_fill_device": (ctypes.c_int, [vp, u64, u64, vp]),
        "adl_synth_probe_queries_device": (ctypes.c_int, [vp, vp, vp, u64, u64, u64, u32, u64, u64, vp]),
        "adl_bloom_profile_enable": (ctypes.c_int, [u32]),
        "adl_bloom_profile_collect": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32)]),
        "adl_bloom_profile_each": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), u32, ctypes.POINTER(u32)]),
        "adl_bloom_test_fault": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64]),
        "adl_bloom_build_positions": (ctypes.c_int, [vp, u32, i32, vp, ctypes.POINTER(u64), vp]),
        "adl_bloom_get_device": (ctypes.c_int, [ctypes.POINTER(i32)]),
        "adl_bloom_set_device": (ctypes.c_int, [i32]),
        "adl_bloom_reload_knobs": (ctypes.c_int, []),
        "adl_bloom_probe_server_launches": (ctypes.c_int, [ctypes.POINTER(u64)]),
        "adl_bloom_probe_server_phases": (ctypes.c_int, [ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                          ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
        "adl_bloom_stream_create": (ctypes.c_int, [u64, ctypes.POINTER(vp)]),
        "adl_bloom_stream_destroy": (ctypes.c_int, [vp]),
        "adl_bloom_stream_reset": (ctypes.c_int, [vp]),
        "adl_bloom_stream_append": (ctypes.c_int, [vp, vp, vp, u64, u32, vp]),
        "adl_bloom_stream_append_device": (ctypes.c_int, [vp, vp, vp, u64, u32, vp]),
        "adl_bloom_stream_cut": (ctypes.c_int, [vp]),
        "adl_bloom_stream_counts": (ctypes.c_int, [vp, ctypes.POINTER(u32), vp, u32]),
        "adl_bloom_stream_finish_workspace_bytes": (u64, [vp, i32]),
        "adl_bloom_stream_finish_device": (ctypes.c_int, [vp, i32, u32, vp, vp, vp, u64, vp]),
        "adl_bloom_stream_finish": (ctypes.c_int, [vp, i32, u32, vp, vp, vp]),
        "adl_bloom_filter_cache_build_stream": (ctypes.c_int, [vp, vp, i32, u32, vp, u64, ctypes.POINTER(u64),
                                                                ctypes.POINTER(vp), vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def reload_knobs() -> None:
    """Re-read the ADL_BLOOM_* switches (the library reads them once per
    process; tests that change them call this, with no call running)."""
    _check(lib().adl_bloom_reload_knobs(), "adl_bloom_reload_knobs")


def _check(status: int, what: str) -> None:
    if status != ADL_OK:
        raise AdlBloomError(status, what)


# ------------------------------------------------------------------ host math
def num_probes(bits_per_key: int) -> int:
    return lib().adl_bloom_num_probes(bits_per_key)


def bitmap_bytes(n: int, bits_per_key: int) -> int:
    return lib().adl_bloom_bitmap_bytes(n, bits_per_key)


def bitmap_alloc_bytes(n: int, bits_per_key: int) -> int:
    return lib().adl_bloom_bitmap_alloc_bytes(n, bits_per_key)


def workspace_bytes(counts, bits_per_key: int) -> int:
    arr = np.ascontiguousarray(counts, dtype=np.uint64)
    return lib().adl_bloom_build_workspace_bytes(arr.ctypes.data, len(arr), bits_per_key)


# ------------------------------------------------------------------ torch plumbing
def _torch():
    import torch
    return torch


def _stream(stream=None):
    torch = _torch()
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def _host_stream(stream=None):
    """`stream` of a host-pointer entry point: None is NULL there, the calling
    thread's own non-blocking stream (include/adl_bloom.h)."""
    return None if stream is None else ctypes.c_void_p(stream.cuda_stream)


def _on(stream):
    """Context in which a wrapper allocates what its call uses on `stream`:
    torch's caching allocator hands memory out per stream -- a block is reused
    only in the order of the stream it was allocated for -- so outputs and
    workspaces are allocated with `stream` current.  Their first use then
    follows whatever used the block before, and a workspace dropped when the
    wrapper returns is reused only behind the call's work, with nothing to
    synchronise.  None: the current stream, as ever."""
    return _torch().cuda.stream(stream)


def _sync(stream=None):
    """Wait for the stream a wrapper was given (None: the current stream)."""
    (_torch().cuda.current_stream() if stream is None else stream).synchronize()


def _dptr(t) -> int | None:
    if t is None:
        return None
    assert t.is_cuda, "device tensor expected"
    return t.data_ptr()


def empty_device(nbytes: int, device="cuda"):
    """uint8 device buffer of nbytes (256-byte aligned by the caching allocator)."""
    return _torch().empty(max(int(nbytes), 1), dtype=_torch().uint8, device=device)


def _keyset(keys, offsets):
    """(keys, offsets) device tensors -> (ptr keys, ptr offs, n, stride)."""
    if offsets is None:
        assert keys.dim() == 2, "fixed-size keys: (n, stride) uint8 tensor"
        return _dptr(keys), None, keys.shape[0], keys.shape[1]
    return _dptr(keys), _dptr(offsets), offsets.numel() - 1, 0


class Builder:
    """Reusable device workspace + bitmap for repeated builds of one shape (bench)."""

    def __init__(self, n: int, bits_per_key: int = 10, device="cuda"):
        self.n, self.bpk = int(n), int(bits_per_key)
        self.nbytes = bitmap_bytes(self.n, self.bpk)
        if self.nbytes == 0:
            raise AdlBloomError(-2, "bitmap size")
        self.bitmap = empty_device(bitmap_alloc_bytes(self.n, self.bpk), device)
        self.ws_bytes = workspace_bytes([self.n], self.bpk)
        self.ws = empty_device(self.ws_bytes, device)

    def positions(self, stream=None) -> int:
        """Positions (bit-sets after repeated pairs were skipped) this builder's last build wrote,
        whatever else the thread has built since.  Pass the build's `stream`: the readback is then
        ordered after the build and needs no synchronise in between."""
        cnt = np.array([self.n], dtype=np.uint64)
        v = ctypes.c_uint64()
        _check(lib().adl_bloom_build_positions(cnt.ctypes.data, 1, self.bpk, _dptr(self.ws), ctypes.byref(v),
                                               _stream(stream)), "adl_bloom_build_positions")
        return v.value

    def build(self, keys, offsets=None, stream=None):
        pk, po, n, stride = _keyset(keys, offsets)
        assert n == self.n
        _check(lib().adl_bloom_build_device(pk, po, n, stride, self.bpk, _dptr(self.bitmap),
                                            _dptr(self.ws), self.ws_bytes, _stream(stream)),
               "adl_bloom_build_device")
        return self.bitmap[: self.nbytes]


class SegmentedBuilder:
    """Reusable buffers for repeated segmented builds (many SSTable filters per launch pair)."""

    def __init__(self, key_begin, bits_per_key: int = 10, device="cuda"):
        self.kb = np.ascontiguousarray(key_begin, dtype=np.uint64)
        self.bpk = int(bits_per_key)
        F = len(self.kb) - 1
        counts = self.kb[1:] - self.kb[:-1]
        self.sizes = np.array([bitmap_bytes(int(c), self.bpk) for c in counts], dtype=np.uint64)
        alloc = np.array([bitmap_alloc_bytes(int(c), self.bpk) for c in counts], dtype=np.uint64)
        self.boff = np.zeros(F, dtype=np.uint64)
        if F > 1:
            self.boff[1:] = np.cumsum(alloc[:-1])
        self.out = empty_device(int(alloc.sum()), device)
        self.ws_bytes = workspace_bytes(counts, self.bpk)
        self.ws = empty_device(self.ws_bytes, device)

    def build(self, keys, offsets=None, stream=None):
        stride = 0 if offsets is not None else keys.shape[1]
        _check(lib().adl_bloom_build_segmented_device(_dptr(keys), _dptr(offsets), stride, self.kb.ctypes.data,
                                                      len(self.kb) - 1, self.bpk, _dptr(self.out),
                                                      self.boff.ctypes.data, _dptr(self.ws), self.ws_bytes,
                                                      _stream(stream)), "adl_bloom_build_segmented_device")
        return self.out

    def positions(self, stream=None) -> int:
        """Positions (bit-sets after repeated pairs were skipped) this builder's last build wrote,
        whatever else the thread has built since.  Pass the build's `stream`: the readback is then
        ordered after the build and needs no synchronise in between."""
        counts = np.ascontiguousarray(self.kb[1:] - self.kb[:-1], dtype=np.uint64)
        v = ctypes.c_uint64()
        _check(lib().adl_bloom_build_positions(counts.ctypes.data, len(counts), self.bpk, _dptr(self.ws),
                                               ctypes.byref(v), _stream(stream)), "adl_bloom_build_positions")
        return v.value

    def bitmap(self, f: int):
        o = int(self.boff[f])
        return self.out[o:o + int(self.sizes[f])]


def build(keys, offsets=None, bits_per_key: int = 10, stream=None):
    """Keys2Block on the GPU: returns the (n*bpk+7)-byte bitmap as a uint8 device tensor."""
    pk, po, n, stride = _keyset(keys, offsets)
    with _on(stream):  # (the workspace is dropped here, with the build perhaps still running)
        b = Builder(n, bits_per_key, keys.device)
    return b.build(keys, offsets, stream)


SKIP_ADJACENT_DUPLICATES = 1
CACHE_VERIFY = 2  # FilterCache.build / build_device: re-probe every build key before the block goes resident


def build_segmented(keys, key_begin, offsets=None, bits_per_key: int = 10, stream=None, flags: int = 0):
    """Many independent filters in one pass pair.  key_begin: host ints (F+1).
    Returns (device bitmaps buffer, host bitmap byte offsets (F), exact sizes (F))."""
    torch = _torch()
    kb = np.ascontiguousarray(key_begin, dtype=np.uint64)
    F = len(kb) - 1
    counts = kb[1:] - kb[:-1]
    sizes = np.array([bitmap_bytes(int(c), bits_per_key) for c in counts], dtype=np.uint64)
    alloc = np.array([bitmap_alloc_bytes(int(c), bits_per_key) for c in counts], dtype=np.uint64)
    boff = np.zeros(F, dtype=np.uint64)
    if F > 1:
        boff[1:] = np.cumsum(alloc[:-1])
    with _on(stream):
        out = empty_device(int(alloc.sum()), keys.device)
    ws_bytes = workspace_bytes(counts, bits_per_key)
    with _on(stream):
        ws = empty_device(ws_bytes, keys.device)
    pk = _dptr(keys)
    po = _dptr(offsets)
    stride = 0 if offsets is not None else keys.shape[1]
    _check(lib().adl_bloom_build_segmented_device_ex(pk, po, stride, kb.ctypes.data, F, bits_per_key,
                                                     _dptr(out), boff.ctypes.data, flags, _dptr(ws), ws_bytes,
                                                     _stream(stream)), "adl_bloom_build_segmented_device_ex")
    _sync(stream)  # ws/out lifetimes end with this call's tensors
    return out, boff, sizes


def filter_block_bytes(key_begin, bits_per_key: int = 10) -> int:
    kb = np.ascontiguousarray(key_begin, dtype=np.uint64)
    return lib().adl_bloom_filter_block_bytes(kb.ctypes.data, len(kb) - 1, bits_per_key)


def build_filter_block(keys, key_begin, offsets=None, bits_per_key: int = 10, stream=None):
    """FilterBlockWriter: Keys2Block() per filter + Final(), framed on the device
    (adl_bloom_filter_block_build_device).  Returns the whole block as a uint8
    device tensor, byte-identical to the reference's."""
    kb = np.ascontiguousarray(key_begin, dtype=np.uint64)
    F = len(kb) - 1
    L = lib()
    nbytes = L.adl_bloom_filter_block_bytes(kb.ctypes.data, F, bits_per_key)
    if nbytes == 0:
        raise AdlBloomError(-2, "filter block size")
    ws_bytes = L.adl_bloom_filter_block_workspace_bytes(kb.ctypes.data, F, bits_per_key)
    dev = keys.device if keys is not None else "cuda"
    with _on(stream):
        block = empty_device(nbytes, dev)
        ws = empty_device(ws_bytes, dev)
    stride = 0 if offsets is not None else (int(keys.shape[1]) if keys is not None else 16)
    _check(L.adl_bloom_filter_block_build_device(_dptr(keys), _dptr(offsets), stride, kb.ctypes.data, F,
                                                 bits_per_key, _dptr(block), nbytes, _dptr(ws), ws_bytes,
                                                 _stream(stream)), "adl_bloom_filter_block_build_device")
    _sync(stream)  # ws lifetime ends with this call
    return block[:nbytes]


def _host_ptr(a):
    """Host address of a numpy array or a CPU (possibly pinned) torch tensor."""
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    assert not a.is_cuda, "host buffer expected"
    return a.data_ptr()


def build_segmented_host(keys, key_begin, out, bitmap_off, offsets=None, bits_per_key: int = 10, stream=None,
                         flags: int = 0):
    """Host-pointer pipelined segmented build (adl_bloom_build_segmented, or
    _ex with flags): keys (n, stride) uint8 or packed bytes + offsets (n+1) in
    host memory (numpy, or CPU torch tensors -- pinned ones are DMAed
    directly); filter f's exact-length bitmap lands at out[bitmap_off[f]:]
    (out: host uint8 buffer)."""
    kb = np.ascontiguousarray(key_begin, dtype=np.uint64)
    bo = np.ascontiguousarray(bitmap_off, dtype=np.uint64)
    stride = 0 if offsets is not None else int(keys.shape[1])
    args = (_host_ptr(keys), None if offsets is None else _host_ptr(offsets), stride, kb.ctypes.data, len(kb) - 1,
            bits_per_key, _host_ptr(out), bo.ctypes.data)
    if flags:
        _check(lib().adl_bloom_build_segmented_ex(*args, flags, _stream(stream)), "adl_bloom_build_segmented_ex")
    else:
        _check(lib().adl_bloom_build_segmented(*args, _stream(stream)), "adl_bloom_build_segmented")
    return out


class StreamBuilder:
    """Streamed build (adl_bloom_stream): keys are appended in batches while a table fills
    (FilterBlockWriter::Update) and hashed on arrival; finish() builds every filter from the stored
    hash pairs (FilterBlockWriter::Final).  One thread at a time per object."""

    def __init__(self, reserve_keys: int = 0):
        self._h = ctypes.c_void_p()
        _check(lib().adl_bloom_stream_create(int(reserve_keys), ctypes.byref(self._h)), "adl_bloom_stream_create")

    def append_status(self, keys, offsets=None, stream=None) -> int:
        """numpy arrays: a host batch (copied before the call returns); torch device tensors: a
        device-resident batch.  keys (n, stride) uint8, or packed bytes with offsets (n + 1) uint64."""
        L = lib()
        if isinstance(keys, np.ndarray):
            if offsets is None:
                assert keys.ndim == 2 and keys.dtype == np.uint8 and keys.flags.c_contiguous
                n, stride, po = keys.shape[0], keys.shape[1], None
            else:
                assert offsets.dtype == np.uint64 and offsets.flags.c_contiguous and keys.flags.c_contiguous
                n, stride, po = len(offsets) - 1, 0, offsets.ctypes.data
            return L.adl_bloom_stream_append(self._h, keys.ctypes.data, po, n, stride, _stream(stream))
        pk, po, n, stride = _keyset(keys, offsets)
        return L.adl_bloom_stream_append_device(self._h, pk, po, n, stride, _stream(stream))

    def append(self, keys, offsets=None, stream=None) -> None:
        _check(self.append_status(keys, offsets, stream), "adl_bloom_stream_append")

    def cut(self) -> None:
        _check(lib().adl_bloom_stream_cut(self._h), "adl_bloom_stream_cut")

    def reset(self) -> None:
        _check(lib().adl_bloom_stream_reset(self._h), "adl_bloom_stream_reset")

    def counts(self) -> np.ndarray:
        """key_begin of the filters so far (F + 1 entries; an open tail counts as a last filter)."""
        nf = ctypes.c_uint32()
        _check(lib().adl_bloom_stream_counts(self._h, ctypes.byref(nf), None, 0), "adl_bloom_stream_counts")
        kb = np.zeros(nf.value + 1, dtype=np.uint64)
        _check(lib().adl_bloom_stream_counts(self._h, ctypes.byref(nf), kb.ctypes.data, len(kb)),
               "adl_bloom_stream_counts")
        return kb

    def workspace_bytes(self, bits_per_key: int = 10) -> int:
        return lib().adl_bloom_stream_finish_workspace_bytes(self._h, bits_per_key)

    def _layout(self, bits_per_key: int):
        kb = self.counts()
        counts = kb[1:] - kb[:-1]
        sizes = np.array([bitmap_bytes(int(c), bits_per_key) for c in counts], dtype=np.uint64)
        alloc = np.array([bitmap_alloc_bytes(int(c), bits_per_key) for c in counts], dtype=np.uint64)
        if len(counts) and (sizes == 0).any():
            raise AdlBloomError(-1 if bits_per_key < 0 else ADL_ERR_TOO_LARGE, "bitmap size")
        boff = np.zeros(len(counts), dtype=np.uint64)
        if len(counts) > 1:
            boff[1:] = np.cumsum(alloc[:-1])
        return boff, sizes, int(alloc.sum())

    def finish(self, bits_per_key: int = 10, flags: int = 0, stream=None, device="cuda"):
        """Every filter's bitmap from the stored pairs, as build_segmented returns them:
        (device bitmaps buffer, host bitmap byte offsets (F), exact sizes (F)).  Enqueued on `stream`
        behind every earlier append; does not synchronise (the workspace is allocated for `stream`)."""
        boff, sizes, total = self._layout(bits_per_key)
        ws_bytes = self.workspace_bytes(bits_per_key)
        with _on(stream):
            out = empty_device(total, device)
            ws = empty_device(ws_bytes, device)
        _check(lib().adl_bloom_stream_finish_device(self._h, bits_per_key, flags, _dptr(out), boff.ctypes.data,
                                                    _dptr(ws), ws_bytes, _stream(stream)),
               "adl_bloom_stream_finish_device")
        return out, boff, sizes

    def finish_host(self, out, bitmap_off, bits_per_key: int = 10, flags: int = 0, stream=None):
        """Filter f's exact-length bitmap into out[bitmap_off[f]:] (host uint8 buffer, any alignment).
        Synchronous."""
        bo = np.ascontiguousarray(bitmap_off, dtype=np.uint64)
        _check(lib().adl_bloom_stream_finish(self._h, bits_per_key, flags, _host_ptr(out), bo.ctypes.data,
                                             _host_stream(stream)), "adl_bloom_stream_finish")
        return out

    def close(self) -> None:
        if self._h:
            lib().adl_bloom_stream_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def probe(keys, bitmap, nbytes: int | None = None, offsets=None, bits_per_key: int = 10, stream=None):
    """IsKeyExists on the GPU for a batch: uint8 device tensor of 0/1."""
    pk, po, n, stride = _keyset(keys, offsets)
    nbytes = bitmap.numel() if nbytes is None else nbytes
    with _on(stream):
        out = _torch().empty(max(n, 1), dtype=_torch().uint8, device=keys.device)
    _check(lib().adl_bloom_probe_device(pk, po, n, stride, bits_per_key, _dptr(bitmap), nbytes,
                                        _dptr(out), _stream(stream)), "adl_bloom_probe_device")
    return out[:n]


def probe_multi(keys, filter_id, bitmaps, bitmap_off, offsets=None, bits_per_key: int = 10, stream=None):
    """Key i against filter filter_id[i]; bitmap_off: device uint64 tensor (F+1)."""
    pk, po, n, stride = _keyset(keys, offsets)
    with _on(stream):
        out = _torch().empty(max(n, 1), dtype=_torch().uint8, device=keys.device)
    _check(lib().adl_bloom_probe_multi_device(pk, po, n, stride, _dptr(filter_id), bitmap_off.numel() - 1,
                                              _dptr(bitmaps), _dptr(bitmap_off), bits_per_key,
                                              _dptr(out), _stream(stream)), "adl_bloom_probe_multi_device")
    return out[:n]


def probe_fanout(keys, pair_begin, pair_filter, bitmaps, bitmap_off, offsets=None, bits_per_key: int = 10, stream=None):
    """Key i against each filter pair_filter[pair_begin[i]:pair_begin[i+1]] (device int32 tensors read as
    uint32: pair_begin has n+1 entries and starts at 0); one answer per pair, in pair order -- probe_multi
    on the expanded pairs, with every key hashed once.  bitmap_off: device uint64 tensor (F+1)."""
    pk, po, n, stride = _keyset(keys, offsets)
    assert pair_begin.numel() == n + 1, "pair_begin: one entry per key and one more"
    npairs = pair_filter.numel()
    with _on(stream):
        out = _torch().empty(max(npairs, 1), dtype=_torch().uint8, device=keys.device)
    _check(lib().adl_bloom_probe_fanout_device(pk, po, n, stride, _dptr(pair_begin), _dptr(pair_filter), npairs,
                                               bitmap_off.numel() - 1, _dptr(bitmaps), _dptr(bitmap_off), None,
                                               bits_per_key, _dptr(out), _stream(stream)),
           "adl_bloom_probe_fanout_device")
    return out[:npairs]


def probe_fanout_hits(keys, pair_begin, pair_filter, bitmaps, bitmap_off, offsets=None, bits_per_key: int = 10,
                      hit_capacity: int | None = None, stream=None):
    """probe_fanout's inputs; only the survivors come back: (hit_begin int32[n+1], hit_filter
    int32[hit_capacity], num_hits int64[1]) device tensors read as unsigned -- key i's hits are
    hit_filter[hit_begin[i]:hit_begin[i+1]], the filters of its pairs answered 1, in pair order.  Enqueued on
    `stream` without a synchronise.  hit_capacity: default the number of pairs."""
    torch = _torch()
    pk, po, n, stride = _keyset(keys, offsets)
    assert pair_begin.numel() == n + 1, "pair_begin: one entry per key and one more"
    npairs = pair_filter.numel()
    cap = npairs if hit_capacity is None else int(hit_capacity)
    wsb = lib().adl_bloom_probe_fanout_hits_workspace_bytes(n, npairs)
    with _on(stream):
        hb = torch.empty(n + 1, dtype=torch.int32, device=keys.device)
        hf = torch.empty(max(cap, 1), dtype=torch.int32, device=keys.device)
        nh = torch.empty(1, dtype=torch.int64, device=keys.device)
        ws = empty_device(wsb, keys.device)
    _check(lib().adl_bloom_probe_fanout_hits_device(pk, po, n, stride, _dptr(pair_begin), _dptr(pair_filter), npairs,
                                                    bitmap_off.numel() - 1, _dptr(bitmaps), _dptr(bitmap_off), None,
                                                    bits_per_key, _dptr(hb), _dptr(hf), cap, _dptr(nh), _dptr(ws),
                                                    wsb, _stream(stream)), "adl_bloom_probe_fanout_hits_device")
    return hb, hf[:cap], nh


def hits_by_table(hit_begin, hit_table, num_tables: int, entry_capacity: int | None = None,
                  group_capacity: int | None = None, stream=None):
    """probe_fanout_hits' output (device int32 tensors read as uint32: hit_begin has n+1 entries) grouped by
    table: (group_table int32[group_capacity], group_begin int32[group_capacity+1], entry_key
    int32[entry_capacity], counts int64[2] = hits H, groups G) device tensors read as unsigned -- the G tables
    with a hit ascending, and entry_key[group_begin[g]:group_begin[g+1]] the keys that hit group_table[g],
    ascending.  Enqueued on `stream` without a synchronise.  entry_capacity: default hit_table's length;
    group_capacity: default min(num_tables, entry_capacity)."""
    torch = _torch()
    n = hit_begin.numel() - 1
    ecap = hit_table.numel() if entry_capacity is None else int(entry_capacity)
    gcap = min(int(num_tables), ecap) if group_capacity is None else int(group_capacity)
    wsb = lib().adl_bloom_hits_by_table_workspace_bytes(n, ecap, num_tables)
    with _on(stream):
        gt = torch.empty(max(gcap, 1), dtype=torch.int32, device=hit_begin.device)
        gbeg = torch.empty(gcap + 1, dtype=torch.int32, device=hit_begin.device)
        ek = torch.empty(max(ecap, 1), dtype=torch.int32, device=hit_begin.device)
        counts = torch.empty(2, dtype=torch.int64, device=hit_begin.device)
        ws = empty_device(wsb, hit_begin.device)
    _check(lib().adl_bloom_hits_by_table_device(_dptr(hit_begin), _dptr(hit_table), n, num_tables, _dptr(gt),
                                                _dptr(gbeg), gcap, _dptr(ek), ecap, _dptr(counts), _dptr(ws), wsb,
                                                _stream(stream)), "adl_bloom_hits_by_table_device")
    return gt[:gcap], gbeg, ek[:ecap], counts


def probe_batch(keys, filter_id, bitmaps, bitmap_off, offsets=None, bits_per_key: int = 10, stream=None,
                bitmap_end=None, out=None):
    """Large-batch multi-filter probe (adl_bloom_probe_batch_device): the answers of
    probe_multi, through the tile-binned pipeline when the batch is large: 16-byte
    keys (an (n, 16) tensor at a 16-byte-aligned address) from 2^20 queries on;
    variable-length keys (`offsets`, n + 1 uint64 from any base) and any other
    stride, at any alignment, from ADL_BLOOM_PROBE_BATCH_VAR_MIN queries on (0:
    never; include/adl_bloom.h).  Every other batch goes to the direct kernel
    inside the call; the answers are the same.  The workspace (sized with
    key_stride 0 for keys with offsets) comes from torch's caching allocator.
    `out`: an optional uint8 device tensor of at least n bytes (any alignment)
    to answer into."""
    pk, po, n, stride = _keyset(keys, offsets)
    F = bitmap_off.numel() - (0 if bitmap_end is not None else 1)
    L = lib()
    wsb = L.adl_bloom_probe_batch_workspace_bytes(n, F, bits_per_key, stride)
    with _on(stream):
        ws = empty_device(wsb, keys.device)
    if out is None:
        with _on(stream):
            out = _torch().empty(max(n, 1), dtype=_torch().uint8, device=keys.device)
    elif out.dtype != _torch().uint8 or out.numel() < n or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of at least n elements")
    _check(L.adl_bloom_probe_batch_device(pk, po, n, stride, _dptr(filter_id), F, _dptr(bitmaps), _dptr(bitmap_off),
                                          _dptr(bitmap_end), bits_per_key, _dptr(out), _dptr(ws), wsb,
                                          _stream(stream)), "adl_bloom_probe_batch_device")
    return out[:n]


def probe_batch_k(keys, filter_id, bitmaps, bitmap_off, filter_k, max_k: int, offsets=None, stream=None,
                  bitmap_end=None, out=None, workspace=None):
    """probe_batch with a probe count per filter (adl_bloom_probe_batch_k_device): filter f
    probes filter_k[f] bits (a uint8 device tensor, one entry per filter, each in [1, max_k]);
    max_k, a host value in 1..30, bounds them and sizes the plan.  Batches, paths and answers
    as probe_batch; a batch whose max_k is above ADL_BLOOM_PROBE_BATCH_MAX_K (default 2; 30: no
    limit) stays on the direct kernel.  `workspace`: an optional uint8 device tensor to use instead of one from torch's
    caching allocator (ADL_ERR_WORKSPACE if the call's plan needs more)."""
    pk, po, n, stride = _keyset(keys, offsets)
    F = bitmap_off.numel() - (0 if bitmap_end is not None else 1)
    if filter_k.dtype != _torch().uint8 or filter_k.numel() < F or not filter_k.is_contiguous():
        raise ValueError("filter_k must be a contiguous uint8 tensor of one entry per filter")
    L = lib()
    if workspace is None:
        wsb = L.adl_bloom_probe_batch_k_workspace_bytes(n, F, max_k, stride)
        with _on(stream):
            workspace = empty_device(wsb, keys.device)
    else:
        wsb = workspace.numel()
    if out is None:
        with _on(stream):
            out = _torch().empty(max(n, 1), dtype=_torch().uint8, device=keys.device)
    elif out.dtype != _torch().uint8 or out.numel() < n or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of at least n elements")
    _check(L.adl_bloom_probe_batch_k_device(pk, po, n, stride, _dptr(filter_id), F, _dptr(bitmaps),
                                            _dptr(bitmap_off), _dptr(bitmap_end), _dptr(filter_k), max_k,
                                            _dptr(out), _dptr(workspace), wsb, _stream(stream)),
           "adl_bloom_probe_batch_k_device")
    return out[:n]


def murmur3_batch(keys, offsets=None, seed_a=SEED1, seed_b=SEED2, stream=None):
    pk, po, n, stride = _keyset(keys, offsets)
    with _on(stream):
        out = _torch().empty((max(n, 1), 2), dtype=_torch().int32, device=keys.device)
    _check(lib().adl_bloom_murmur3_device(pk, po, n, stride, seed_a, seed_b, _dptr(out), _stream(stream)),
           "adl_bloom_murmur3_device")
    return out[:n]


def murmur3(seed: int, data: bytes) -> int:
    """murmur3_hash(seed, data, len) evaluated on the GPU."""
    buf = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    h = ctypes.c_uint32(0)
    _check(lib().adl_bloom_murmur3(seed, ctypes.cast(buf, ctypes.c_void_p), len(data), ctypes.byref(h)),
           "adl_bloom_murmur3")
    return h.value


# test-only fault injection (include/adl_bloom.h, adl_bloom_test_fault)
TEST_FAULT_PIPELINE_GROUP = 1
TEST_FAULT_CACHE_COMPLETION = 2
TEST_FAULT_CACHE_BUILD_CORRUPT = 3
TEST_FAULT_SERVER_SEQ = 4  # no failure: presets the calling thread's next probe-server sequence number


def test_fault(site: int, arg: int) -> None:
    """Arm (arg >= 0) or disarm (arg < 0) a one-shot injected failure."""
    _check(lib().adl_bloom_test_fault(site, arg), "adl_bloom_test_fault")


def probe_server_launches() -> int:
    """Probe-server kernels this process has launched (relaunches included)."""
    n = ctypes.c_uint64(0)
    _check(lib().adl_bloom_probe_server_launches(ctypes.byref(n)), "adl_bloom_probe_server_launches")
    return n.value


def probe_server_phases(reset: bool = False):
    """(requests served by a resident probe server, of them stamped, avg_us[7]) since the last reset
    (adl_bloom_probe_server_phases).  A request that fell back to a launched probe is not counted."""
    n, st = ctypes.c_uint64(0), ctypes.c_uint64(0)
    avg = (ctypes.c_double * 7)()
    _check(lib().adl_bloom_probe_server_phases(ctypes.byref(n), ctypes.byref(st), avg, int(reset)),
           "adl_bloom_probe_server_phases")
    return n.value, st.value, list(avg)


def profile_enable(capacity: int = 4096) -> None:
    """Start per-kernel HIP-event timing of builds issued by this thread."""
    _check(lib().adl_bloom_profile_enable(capacity), "adl_bloom_profile_enable")


def profile_each(capacity: int = 4096):
    """-> [(pass A ms, pass B ms)] per timed launch pair so far (timing keeps running)."""
    buf = (ctypes.c_double * (2 * capacity))()
    n = ctypes.c_uint32(0)
    _check(lib().adl_bloom_profile_each(buf, capacity, ctypes.byref(n)), "adl_bloom_profile_each")
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n.value)]


def profile_collect():
    """-> (pass A ms summed, pass B ms summed, builds timed); stops timing."""
    ms = (ctypes.c_double * 2)()
    nb = ctypes.c_uint32(0)
    _check(lib().adl_bloom_profile_collect(ms, ctypes.byref(nb)), "adl_bloom_profile_collect")
    return ms[0], ms[1], nb.value


# ------------------------------------------------------------------ host-pointer API
def build_host(keys: np.ndarray, offsets: np.ndarray | None = None, bits_per_key: int = 10,
               out: np.ndarray | None = None, stream=None) -> np.ndarray:
    """adl_bloom_build: host keys in, host bitmap out (upload + build + download).
    `stream` (here and in the other host-pointer wrappers): a torch stream to run
    on, or None for the calling thread's own non-blocking stream.
    `out`: an optional uint8 host array (any alignment; pinned or pageable) of
    at least the bitmap's size to write it into."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    if offsets is None:
        n, stride, po = keys.shape[0], keys.shape[1], None
    else:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, stride, po = len(offsets) - 1, 0, offsets.ctypes.data
    nb = bitmap_bytes(n, bits_per_key)
    if nb == 0:
        raise AdlBloomError(-2, "bitmap size")
    if out is None:
        out = np.empty(nb, dtype=np.uint8)
    elif out.dtype != np.uint8 or out.size < nb or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("out must be a contiguous uint8 array of at least the bitmap's size")
    kp = keys.ctypes.data if keys.size else np.zeros(1, np.uint8).ctypes.data
    _check(lib().adl_bloom_build(kp, po, n, stride, bits_per_key, out.ctypes.data, _host_stream(stream)),
           "adl_bloom_build")
    return out[:nb]


def probe_host(keys: np.ndarray, bitmap: np.ndarray, offsets: np.ndarray | None = None,
               bits_per_key: int = 10, stream=None) -> np.ndarray:
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
    if offsets is None:
        n, stride, po = keys.shape[0], keys.shape[1], None
    else:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, stride, po = len(offsets) - 1, 0, offsets.ctypes.data
    out = np.empty(max(n, 1), dtype=np.uint8)
    _check(lib().adl_bloom_probe(keys.ctypes.data, po, n, stride, bits_per_key, bitmap.ctypes.data,
                                 bitmap.size, out.ctypes.data, _host_stream(stream)), "adl_bloom_probe")
    return out[:n]


class FilterSet:
    """Device-resident bitmaps (adl_bloom_filter_set): the reader side."""

    def __init__(self, bitmaps: np.ndarray, bitmap_off: np.ndarray, bits_per_key: int = 10):
        bitmaps = np.ascontiguousarray(bitmaps, dtype=np.uint8)
        off = np.ascontiguousarray(bitmap_off, dtype=np.uint64)
        self._h = ctypes.c_void_p()
        _check(lib().adl_bloom_filter_set_create(bitmaps.ctypes.data, off.ctypes.data, len(off) - 1,
                                                 bits_per_key, ctypes.byref(self._h)),
               "adl_bloom_filter_set_create")

    def probe(self, keys: np.ndarray, filter_id=None, filter: int = 0, offsets=None, stream=None) -> np.ndarray:
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        if offsets is None:
            n, stride, po = keys.shape[0], keys.shape[1], None
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n, stride, po = len(offsets) - 1, 0, offsets.ctypes.data
        fid = None if filter_id is None else np.ascontiguousarray(filter_id, dtype=np.uint32)
        out = np.empty(max(n, 1), dtype=np.uint8)
        _check(lib().adl_bloom_filter_set_probe(self._h, keys.ctypes.data, po, n, stride,
                                                None if fid is None else fid.ctypes.data, filter,
                                                out.ctypes.data, _host_stream(stream)), "adl_bloom_filter_set_probe")
        return out[:n]

    def close(self):
        if self._h:
            lib().adl_bloom_filter_set_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_keys(keys, offsets):
    """Host keys (and offsets) as the C-ABI takes them: (arrays to keep alive, key pointer, offsets pointer or
    None, n, stride).  A batch of no key bytes still has an address."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    if offsets is None:
        n, stride, po = keys.shape[0], keys.shape[1], None
    else:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, stride, po = len(offsets) - 1, 0, offsets.ctypes.data
    kbuf = keys if keys.size else np.zeros(16, np.uint8)
    return (kbuf, offsets), kbuf.ctypes.data, po, n, stride


class FilterCache:
    """Device-resident filter blocks keyed by SSTable oid, LRU (adl_bloom_filter_cache)."""

    def __init__(self, capacity_bytes: int, max_tables: int = 64, bits_per_key: int = 10):
        self._h = ctypes.c_void_p()
        _check(lib().adl_bloom_filter_cache_create(capacity_bytes, max_tables, bits_per_key, ctypes.byref(self._h)),
               "adl_bloom_filter_cache_create")

    def put(self, oid: bytes, block: bytes) -> None:
        b = np.frombuffer(block, dtype=np.uint8)
        _check(lib().adl_bloom_filter_cache_put(self._h, oid, len(oid), b.ctypes.data, b.size),
               "adl_bloom_filter_cache_put")

    def put_status(self, oid: bytes, block: bytes) -> int:
        b = np.frombuffer(block, dtype=np.uint8)
        return lib().adl_bloom_filter_cache_put(self._h, oid, len(oid), b.ctypes.data, b.size)

    def __contains__(self, oid: bytes) -> bool:
        return lib().adl_bloom_filter_cache_contains(self._h, oid, len(oid)) == 1

    def remove(self, oid: bytes) -> bool:
        return lib().adl_bloom_filter_cache_remove(self._h, oid, len(oid)) == 1

    def stats(self):
        t, b = ctypes.c_uint32(), ctypes.c_uint64()
        _check(lib().adl_bloom_filter_cache_stats(self._h, ctypes.byref(t), ctypes.byref(b)), "stats")
        return t.value, b.value

    def probe(self, oids, table, keys: np.ndarray, offsets=None, filter: int = 0, stream=None):
        """Query i against filter `filter` of table oids[table[i]]; returns (0/1 array, uncached count)."""
        keep, kp, po, n, stride = _host_keys(keys, offsets)
        arr = (ctypes.c_char_p * max(len(oids), 1))(*oids)
        lens = np.array([len(o) for o in oids] or [0], dtype=np.uint64)
        tab = np.ascontiguousarray(table, dtype=np.uint32)
        out = np.empty(max(n, 1), dtype=np.uint8)
        unc = ctypes.c_uint64()
        _check(lib().adl_bloom_filter_cache_probe(self._h, arr, lens.ctypes.data, len(oids), filter,
                                                  kp, po, n, stride, tab.ctypes.data,
                                                  out.ctypes.data, ctypes.byref(unc), _host_stream(stream)),
               "adl_bloom_filter_cache_probe")
        return out[:n], unc.value

    def probe_batch_workspace_bytes(self, oids, n: int, key_stride: int) -> int:
        """The workspace probe_batch_device needs for n queries over `oids` as they are cached now
        (key_stride 0: keys with offsets)."""
        arr = (ctypes.c_char_p * max(len(oids), 1))(*oids)
        lens = np.array([len(o) for o in oids] or [0], dtype=np.uint64)
        return lib().adl_bloom_filter_cache_probe_batch_workspace_bytes(self._h, arr, lens.ctypes.data, len(oids), n,
                                                                        key_stride)

    def probe_batch_device_status(self, oids, table, keys, offsets=None, filter: int = 0, stream=None, out=None,
                                  workspace=None):
        """probe_batch_device that returns (status, out, cached) instead of raising."""
        pk, po, n, stride = _keyset(keys, offsets)
        arr = (ctypes.c_char_p * max(len(oids), 1))(*oids)
        lens = np.array([len(o) for o in oids] or [0], dtype=np.uint64)
        L = lib()
        if workspace is None:
            wsb = L.adl_bloom_filter_cache_probe_batch_workspace_bytes(self._h, arr, lens.ctypes.data, len(oids), n,
                                                                       stride)
            with _on(stream):
                workspace = empty_device(wsb, keys.device)
        else:
            wsb = workspace.numel()
        if out is None:
            with _on(stream):
                out = _torch().empty(max(n, 1), dtype=_torch().uint8, device=keys.device)
        elif out.dtype != _torch().uint8 or out.numel() < n or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor of at least n elements")
        cached = np.zeros(max(len(oids), 1), dtype=np.uint8)
        rc = L.adl_bloom_filter_cache_probe_batch_device(self._h, arr, lens.ctypes.data, len(oids), filter, pk, po, n,
                                                         stride, _dptr(table), _dptr(out), cached.ctypes.data,
                                                         _dptr(workspace), wsb, _stream(stream))
        return rc, out[:n], cached[:len(oids)]

    def probe_batch_device(self, oids, table, keys, offsets=None, filter: int = 0, stream=None, out=None,
                           workspace=None):
        """Bulk probe of DEVICE keys (adl_bloom_filter_cache_probe_batch_device): query i against filter `filter`
        of table oids[table[i]] (`table`: a uint32 device tensor), each table with the k of its own block, through
        the tile-binned pipeline when the batch is large.  Returns (0/1 uint8 device tensor, per-table cached
        flags as a numpy array); the answers are probe()'s, and an index >= len(oids) answers 0.  The call
        returns after the probe has completed on `stream`."""
        rc, out, cached = self.probe_batch_device_status(oids, table, keys, offsets, filter, stream, out, workspace)
        _check(rc, "adl_bloom_filter_cache_probe_batch_device")
        return out, cached

    def probe_fanout(self, oids, pair_begin, pair_table, keys: np.ndarray, offsets=None, filter: int = 0,
                     stream=None):
        """Key i against filter `filter` of every table oids[t], t in pair_table[pair_begin[i]:pair_begin[i+1]];
        returns (0/1 per pair in pair order, uncached pair count): probe() on the expanded pairs, each key
        uploaded and hashed once."""
        keep, kp, po, n, stride = _host_keys(keys, offsets)
        arr = (ctypes.c_char_p * max(len(oids), 1))(*oids)
        lens = np.array([len(o) for o in oids] or [0], dtype=np.uint64)
        pb = np.ascontiguousarray(pair_begin, dtype=np.uint32)
        tab = np.ascontiguousarray(pair_table, dtype=np.uint32)
        if len(pb) != n + 1:
            raise ValueError("pair_begin needs one entry per key and one more")
        if len(pb) and int(pb[-1]) != len(tab):
            raise ValueError("pair_begin[-1] must equal len(pair_table)")
        out = np.empty(max(len(tab), 1), dtype=np.uint8)
        unc = ctypes.c_uint64()
        _check(lib().adl_bloom_filter_cache_probe_fanout(self._h, arr, lens.ctypes.data, len(oids), filter, kp, po,
                                                         n, stride, pb.ctypes.data, tab.ctypes.data, out.ctypes.data,
                                                         ctypes.byref(unc), _host_stream(stream)),
               "adl_bloom_filter_cache_probe_fanout")
        return out[:len(tab)], unc.value

    def probe_key(self, oids, key: bytes, filter: int = 0, stream=None):
        """ONE key against filter `filter` of every table in oids (adl_bloom_filter_cache_probe_key): (0/1 per
        table, uncached count) -- probe_fanout for one key with all the tables as its list.  Up to GET_MAX_TABLES
        tables and GET_MAX_KEY_BYTES key bytes are one request to the resident server, with no launch."""
        key = bytes(key)
        kb = np.frombuffer(key, dtype=np.uint8) if key else np.zeros(1, np.uint8)
        arr = (ctypes.c_char_p * max(len(oids), 1))(*oids)
        lens = np.array([len(o) for o in oids] or [0], dtype=np.uint64)
        out = np.empty(max(len(oids), 1), dtype=np.uint8)
        unc = ctypes.c_uint64()
        _check(lib().adl_bloom_filter_cache_probe_key(self._h, arr, lens.ctypes.data, len(oids), filter,
                                                      kb.ctypes.data, len(key), out.ctypes.data, ctypes.byref(unc),
                                                      _host_stream(stream)),
               "adl_bloom_filter_cache_probe_key")
        return out[:len(oids)], unc.value

    # ---- write-through: a table's filter block built straight into the arena
    class Ticket:
        """A built, unpublished block (adl_bloom_cache_ticket): publish or abandon it.
        `block`: device variant only, the host tensor the block is copied into
        (complete once publish, abandon or a stream synchronise has returned)."""

        def __init__(self, handle, keep=(), block=None, nbytes=0):
            self._h, self._keep, self.block, self.nbytes = handle, keep, block, nbytes

        def block_bytes(self) -> bytes:
            return bytes(self.block[:self.nbytes].numpy().tobytes())

    def build_status(self, keys, key_begin, offsets=None, bits_per_key: int = 10, flags: int = 0, stream=None):
        """adl_bloom_filter_cache_build on host numpy keys: (status, block bytes or None, ticket or None)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        kb = np.ascontiguousarray(key_begin, dtype=np.uint64)
        if offsets is None:
            stride, po = (int(keys.shape[1]) if keys.ndim == 2 else 16), None
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            stride, po = 0, offsets.ctypes.data
        nbytes = lib().adl_bloom_filter_block_bytes(kb.ctypes.data, len(kb) - 1, bits_per_key)
        block = np.empty(max(nbytes, 1), dtype=np.uint8)
        kp = keys.ctypes.data if keys.size else np.zeros(16, np.uint8).ctypes.data
        h = ctypes.c_void_p()
        rc = lib().adl_bloom_filter_cache_build(self._h, kp, po, stride, kb.ctypes.data, len(kb) - 1, bits_per_key,
                                                flags, block.ctypes.data, nbytes, ctypes.byref(h),
                                                _host_stream(stream))
        if rc != ADL_OK:
            return rc, None, None
        return rc, block[:nbytes].tobytes(), FilterCache.Ticket(h)

    def build(self, keys, key_begin, offsets=None, bits_per_key: int = 10, flags: int = 0, stream=None):
        """Build the filter block of keys (filter f = keys [key_begin[f], key_begin[f+1])) into a reserved
        range of the arena: returns (block: bytes, ticket).  The block is the reference's, for the file;
        publish(ticket, oid) makes it resident under the table's oid, abandon(ticket) gives the range back."""
        rc, block, t = self.build_status(keys, key_begin, offsets, bits_per_key, flags, stream)
        _check(rc, "adl_bloom_filter_cache_build")
        return block, t

    def build_stream_status(self, sb: "StreamBuilder", bits_per_key: int = 10, flags: int = 0, stream=None):
        """(status, block bytes or None, ticket or None) of adl_bloom_filter_cache_build_stream."""
        nbytes = filter_block_bytes(sb.counts(), bits_per_key)
        if nbytes == 0:
            return (-1 if bits_per_key < 0 else ADL_ERR_TOO_LARGE), None, None
        block = np.empty(nbytes, dtype=np.uint8)
        h, got = ctypes.c_void_p(), ctypes.c_uint64()
        rc = lib().adl_bloom_filter_cache_build_stream(self._h, sb._h, bits_per_key, flags, block.ctypes.data, nbytes,
                                                       ctypes.byref(got), ctypes.byref(h), _host_stream(stream))
        if rc != ADL_OK:
            return rc, None, None
        return rc, block[:got.value].tobytes(), FilterCache.Ticket(h)

    def build_stream(self, sb: "StreamBuilder", bits_per_key: int = 10, flags: int = 0, stream=None):
        """build() with a StreamBuilder as the key source: the filters of sb.counts() built from its hash
        pairs into a reserved range of the arena (nothing is uploaded or hashed); returns (block: bytes,
        ticket) for publish / abandon.  CACHE_VERIFY re-probes from the pairs.  `sb` is not consumed."""
        rc, block, t = self.build_stream_status(sb, bits_per_key, flags, stream)
        _check(rc, "adl_bloom_filter_cache_build_stream")
        return block, t

    def build_device(self, keys, key_begin, offsets=None, bits_per_key: int = 10, flags: int = 0, stream=None,
                     h_block="pinned"):
        """The same from torch device tensors, enqueued on `stream` without a synchronise; the workspace
        comes from torch's caching allocator and lives with the ticket.  h_block: a pinned CPU uint8 tensor
        to receive the block, "pinned" to allocate one, or None for no download.  Returns the ticket
        (ticket.block: that tensor)."""
        torch = _torch()
        kb = np.ascontiguousarray(key_begin, dtype=np.uint64)
        L = lib()
        nbytes = L.adl_bloom_filter_block_bytes(kb.ctypes.data, len(kb) - 1, bits_per_key)
        wsb = L.adl_bloom_filter_cache_build_workspace_bytes(kb.ctypes.data, len(kb) - 1, bits_per_key)
        if nbytes == 0 or wsb == 0:
            raise AdlBloomError(-2, "filter block size")
        with _on(stream):
            ws = empty_device(wsb, keys.device if keys is not None else "cuda")
        if isinstance(h_block, str):
            h_block = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        stride = 0 if offsets is not None else (int(keys.shape[1]) if keys is not None else 16)
        h = ctypes.c_void_p()
        _check(L.adl_bloom_filter_cache_build_device(self._h, _dptr(keys), _dptr(offsets), stride, kb.ctypes.data,
                                                     len(kb) - 1, bits_per_key, flags, _dptr(ws), wsb,
                                                     None if h_block is None else h_block.data_ptr(),
                                                     0 if h_block is None else h_block.numel(), ctypes.byref(h),
                                                     _stream(stream)), "adl_bloom_filter_cache_build_device")
        return FilterCache.Ticket(h, (ws, keys, offsets), h_block, nbytes)

    def publish_status(self, ticket, oid: bytes) -> int:
        h, ticket._h, keep = ticket._h, None, ticket._keep
        rc = lib().adl_bloom_filter_cache_publish(self._h, h, oid, len(oid))
        del keep  # (the build's work has ended: publish waited for it)
        ticket._keep = ()
        return rc

    def publish(self, ticket, oid: bytes) -> None:
        _check(self.publish_status(ticket, oid), "adl_bloom_filter_cache_publish")

    def abandon(self, ticket) -> None:
        h, ticket._h = ticket._h, None
        _check(lib().adl_bloom_filter_cache_abandon(self._h, h), "adl_bloom_filter_cache_abandon")
        ticket._keep = ()

    def build_put(self, oid: bytes, keys, key_begin, offsets=None, bits_per_key: int = 10, flags: int = 0) -> bytes:
        """build + publish under `oid`; returns the block."""
        block, t = self.build(keys, key_begin, offsets, bits_per_key, flags)
        self.publish(t, oid)
        return block

    def close(self):
        if self._h:
            lib().adl_bloom_filter_cache_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ADL_ERR_TOO_LARGE = -2
ADL_ERR_WORKSPACE = -5


def _ptr_array(items):
    """list[bytes] -> (char*[] kept alive by the caller, lengths u64)."""
    arr = (ctypes.c_char_p * max(len(items), 1))(*items)
    return arr, np.array([len(b) for b in items] or [0], dtype=np.uint64)


class LevelIndex:
    """A level's resident index (adl_bloom_level): built once from the tables' (min, max) inner keys,
    asked about many times.  tables: [(min_inner_key, max_inner_key)]; oids: their cache keys (needed by
    multiget only).  Raises AdlBloomError(ADL_ERR_TOO_LARGE) when the index would exceed max_index_bytes
    (0: 256 MiB)."""

    def __init__(self, tables, oids=None, max_index_bytes: int = 0):
        self._h = ctypes.c_void_p()
        self.num_tables = len(tables)
        mins, ml = _ptr_array([bytes(t[0]) for t in tables])
        maxs, xl = _ptr_array([bytes(t[1]) for t in tables])
        po, ol = (None, None) if oids is None else _ptr_array([bytes(o) for o in oids])
        if oids is not None and len(oids) != len(tables):
            raise ValueError("one oid per table")
        _check(lib().adl_bloom_level_create(None if po is None else ctypes.cast(po, ctypes.c_void_p),
                                            None if ol is None else ol.ctypes.data,
                                            ctypes.cast(mins, ctypes.c_void_p), ml.ctypes.data,
                                            ctypes.cast(maxs, ctypes.c_void_p), xl.ctypes.data, len(tables),
                                            max_index_bytes, ctypes.byref(self._h)), "adl_bloom_level_create")

    def stats(self):
        """-> (regions, list entries, device bytes, longest candidate list)."""
        r, lg = ctypes.c_uint32(), ctypes.c_uint32()
        e, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().adl_bloom_level_stats(self._h, ctypes.byref(r), ctypes.byref(e), ctypes.byref(b),
                                           ctypes.byref(lg)), "adl_bloom_level_stats")
        return r.value, e.value, b.value, lg.value

    def candidates_device(self, keys, offsets=None, seq: int = 2**63 - 1, pair_capacity: int | None = None,
                          stream=None):
        """Selection on the device from torch device tensors, enqueued on `stream` without a synchronise:
        (pair_begin int32[n+1], pair_table int32[pair_capacity], num_pairs int64[1]) device tensors, read as
        unsigned.  pair_capacity: default n * the longest list."""
        torch = _torch()
        pk, po, n, stride = _keyset(keys, offsets)
        cap = n * self.stats()[3] if pair_capacity is None else int(pair_capacity)
        wsb = lib().adl_bloom_level_candidates_workspace_bytes(n)
        with _on(stream):
            pb = torch.empty(n + 1, dtype=torch.int32, device=keys.device)
            pt = torch.empty(max(cap, 1), dtype=torch.int32, device=keys.device)
            npairs = torch.empty(1, dtype=torch.int64, device=keys.device)
            ws = empty_device(wsb, keys.device)
        _check(lib().adl_bloom_level_candidates_device(self._h, pk, po, n, stride, seq, _dptr(pb), _dptr(pt), cap,
                                                       _dptr(npairs), _dptr(ws), wsb, _stream(stream)),
               "adl_bloom_level_candidates_device")
        return pb, pt[:cap], npairs

    def multiget_status(self, cache: "FilterCache", keys: np.ndarray, offsets=None, seq: int = 2**63 - 1,
                        filter: int = 0, pair_capacity: int | None = None, stream=None):
        """adl_bloom_level_multiget: (status, pair_begin, pair_table, answers, num_pairs, uncached)."""
        keep, kp, po, n, stride = _host_keys(keys, offsets)
        cap = n * self.stats()[3] if pair_capacity is None else int(pair_capacity)
        pb = np.zeros(n + 1, dtype=np.uint32)
        pt = np.zeros(max(cap, 1), dtype=np.uint32)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        npairs, unc = ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib().adl_bloom_level_multiget(self._h, cache._h, filter, kp, po, n, stride, seq, pb.ctypes.data,
                                            pt.ctypes.data, out.ctypes.data, cap, ctypes.byref(npairs),
                                            ctypes.byref(unc), _host_stream(stream))
        m = min(npairs.value, cap)
        return rc, pb, pt[:m], out[:m], npairs.value, unc.value

    def multiget(self, cache: "FilterCache", keys: np.ndarray, offsets=None, seq: int = 2**63 - 1, filter: int = 0,
                 stream=None):
        """Level multi-get: keys up; selection, expansion and probes on the device;
        (pair_begin, pair_table, answers, uncached) back."""
        rc, pb, pt, out, _, unc = self.multiget_status(cache, keys, offsets, seq, filter, None, stream)
        _check(rc, "adl_bloom_level_multiget")
        return pb, pt, out, unc

    def close(self):
        if self._h:
            lib().adl_bloom_level_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Revision:
    """A revision (adl_bloom_revision): its levels' LevelIndex objects in Revision::Get's visiting order, level 0
    first; None or a level of no tables is an empty level.  The levels are borrowed (this object keeps them
    alive).  Every call reports GLOBAL table ids: table t of level l is stats()[1][l] + t."""

    def __init__(self, levels):
        self._h = ctypes.c_void_p()
        self._levels = list(levels)
        arr = (ctypes.c_void_p * max(len(self._levels), 1))(*[None if lv is None else lv._h.value
                                                             for lv in self._levels])
        _check(lib().adl_bloom_revision_create(ctypes.cast(arr, ctypes.c_void_p), len(self._levels),
                                               ctypes.byref(self._h)), "adl_bloom_revision_create")

    def stats(self):
        """-> (levels, table_base uint32[levels + 1], the longest candidate list over all levels)."""
        nl, lg = ctypes.c_uint32(), ctypes.c_uint32()
        base = np.zeros(len(self._levels) + 1, dtype=np.uint32)
        _check(lib().adl_bloom_revision_stats(self._h, ctypes.byref(nl), base.ctypes.data, ctypes.byref(lg)),
               "adl_bloom_revision_stats")
        return nl.value, base, lg.value

    def candidates_device(self, keys, offsets=None, seq: int = 2**63 - 1, pair_capacity: int | None = None,
                          stream=None):
        """Selection over every level on the device from torch device tensors, enqueued on `stream` without a
        synchronise: (pair_begin int32[n+1], pair_table int32[pair_capacity], num_pairs int64[1]) device
        tensors, read as unsigned.  pair_capacity: default n * the longest list."""
        torch = _torch()
        pk, po, n, stride = _keyset(keys, offsets)
        cap = n * self.stats()[2] if pair_capacity is None else int(pair_capacity)
        wsb = lib().adl_bloom_revision_candidates_workspace_bytes(self._h, n)
        with _on(stream):
            pb = torch.empty(n + 1, dtype=torch.int32, device=keys.device)
            pt = torch.empty(max(cap, 1), dtype=torch.int32, device=keys.device)
            npairs = torch.empty(1, dtype=torch.int64, device=keys.device)
            ws = empty_device(wsb, keys.device)
        _check(lib().adl_bloom_revision_candidates_device(self._h, pk, po, n, stride, seq, _dptr(pb), _dptr(pt), cap,
                                                          _dptr(npairs), _dptr(ws), wsb, _stream(stream)),
               "adl_bloom_revision_candidates_device")
        return pb, pt[:cap], npairs

    def multiget_status(self, cache: "FilterCache", keys: np.ndarray, offsets=None, seq: int = 2**63 - 1,
                        filter: int = 0, hit_capacity: int | None = None, pair_capacity: int = 0, stream=None):
        """adl_bloom_revision_multiget: (status, hit_begin, hit_table, num_hits, num_pairs, uncached).
        hit_capacity: default n * the longest list."""
        keep, kp, po, n, stride = _host_keys(keys, offsets)
        cap = n * self.stats()[2] if hit_capacity is None else int(hit_capacity)
        hb = np.zeros(n + 1, dtype=np.uint32)
        ht = np.zeros(max(cap, 1), dtype=np.uint32)
        nh, npairs, unc = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib().adl_bloom_revision_multiget(self._h, cache._h, filter, kp, po, n, stride, seq, hb.ctypes.data,
                                               ht.ctypes.data, cap, ctypes.byref(nh), int(pair_capacity),
                                               ctypes.byref(npairs), ctypes.byref(unc), _host_stream(stream))
        return rc, hb, ht[:min(nh.value, cap)], nh.value, npairs.value, unc.value

    def multiget(self, cache: "FilterCache", keys: np.ndarray, offsets=None, seq: int = 2**63 - 1, filter: int = 0,
                 stream=None):
        """Revision multi-get: keys up; selection over every level, probes and compaction on the device;
        (hit_begin, hit_table, uncached) back -- per key the tables still to read, in visiting order."""
        rc, hb, ht, _, _, unc = self.multiget_status(cache, keys, offsets, seq, filter, None, 0, stream)
        _check(rc, "adl_bloom_revision_multiget")
        return hb, ht, unc

    def candidates_host(self, key: bytes, seq: int = 2**63 - 1, capacity: int | None = None):
        """One key's candidate tables over all levels from the levels' host indices, no GPU
        (adl_bloom_revision_candidates_host): (global ids uint32 in visiting order, their total).  capacity:
        default the longest list; entries beyond it are not reported."""
        key = bytes(key)
        kb = np.frombuffer(key, dtype=np.uint8) if key else np.zeros(1, np.uint8)
        cap = self.stats()[2] if capacity is None else int(capacity)
        tab = np.full(max(cap, 1), 0xA5A5A5A5, dtype=np.uint32)
        num = ctypes.c_uint32()
        _check(lib().adl_bloom_revision_candidates_host(self._h, kb.ctypes.data, len(key), seq, tab.ctypes.data, cap,
                                                        ctypes.byref(num)), "adl_bloom_revision_candidates_host")
        return tab[:min(num.value, cap)], num.value

    def get_status(self, cache: "FilterCache", key: bytes, seq: int = 2**63 - 1, filter: int = 0,
                   hit_capacity: int | None = None, stream=None):
        """adl_bloom_revision_get: (status, hit_table, num_hits, num_candidates, uncached).  hit_capacity:
        default the longest list.  The array starts as 0xA5 bytes; without status 0 nothing is written to it."""
        key = bytes(key)
        kb = np.frombuffer(key, dtype=np.uint8) if key else np.zeros(1, np.uint8)
        cap = self.stats()[2] if hit_capacity is None else int(hit_capacity)
        ht = np.full(max(cap, 1), 0xA5A5A5A5, dtype=np.uint32)
        nh, nc, unc = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        rc = lib().adl_bloom_revision_get(self._h, cache._h, filter, kb.ctypes.data, len(key), seq, ht.ctypes.data,
                                          cap, ctypes.byref(nh), ctypes.byref(nc), ctypes.byref(unc),
                                          _host_stream(stream))
        return rc, ht[:min(nh.value, cap)] if rc == ADL_OK else ht[:cap], nh.value, nc.value, unc.value

    def get(self, cache: "FilterCache", key: bytes, seq: int = 2**63 - 1, filter: int = 0, stream=None):
        """Revision Get of one key -- DB::Get's filter stage: (hit_table, uncached), the tables still to read as
        global ids in visiting order; multiget's list for that key.  The candidates are selected on the host and
        asked about in ONE request to the cache's resident server (no launch) when they are at most
        GET_MAX_TABLES and the key at most GET_MAX_KEY_BYTES bytes; otherwise one launched fan-out probe."""
        rc, ht, _, _, unc = self.get_status(cache, key, seq, filter, None, stream)
        _check(rc, "adl_bloom_revision_get")
        return ht, unc

    def read_plan_status(self, cache: "FilterCache", keys: np.ndarray, offsets=None, seq: int = 2**63 - 1,
                         filter: int = 0, entry_capacity: int | None = None, group_capacity: int | None = None,
                         pair_capacity: int = 0, stream=None):
        """adl_bloom_revision_read_plan: (status, group_table, group_begin, entry_key, num_groups, num_hits,
        num_pairs, uncached).  entry_capacity: default n * the longest list; group_capacity: default the
        revision's tables.  The arrays start as 0xA5 bytes; without status 0 nothing is written to them."""
        keep, kp, po, n, stride = _host_keys(keys, offsets)
        _, base, longest = self.stats()
        ecap = n * longest if entry_capacity is None else int(entry_capacity)
        gcap = int(base[-1]) if group_capacity is None else int(group_capacity)
        gt = np.full(max(gcap, 1), 0xA5A5A5A5, dtype=np.uint32)
        gbeg = np.full(gcap + 1, 0xA5A5A5A5, dtype=np.uint32)
        ek = np.full(max(ecap, 1), 0xA5A5A5A5, dtype=np.uint32)
        ng, nh, npairs, unc = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib().adl_bloom_revision_read_plan(self._h, cache._h, filter, kp, po, n, stride, seq, gt.ctypes.data,
                                                gbeg.ctypes.data, gcap, ctypes.byref(ng), ek.ctypes.data, ecap,
                                                ctypes.byref(nh), int(pair_capacity), ctypes.byref(npairs),
                                                ctypes.byref(unc), _host_stream(stream))
        if rc == ADL_OK:
            gt, gbeg, ek = gt[:ng.value], gbeg[:ng.value + 1], ek[:nh.value]
        return rc, gt, gbeg, ek, ng.value, nh.value, npairs.value, unc.value

    def read_plan(self, cache: "FilterCache", keys: np.ndarray, offsets=None, seq: int = 2**63 - 1, filter: int = 0,
                  stream=None):
        """Revision multi-get as a read plan: (group_table, group_begin, entry_key, uncached) -- the tables to
        open, global ids ascending (the levels ascending), and for table group_table[g] the indices of the
        batch's keys to look up in it, entry_key[group_begin[g]:group_begin[g+1]], ascending."""
        rc, gt, gbeg, ek, _, _, _, unc = self.read_plan_status(cache, keys, offsets, seq, filter, None, None, 0,
                                                               stream)
        _check(rc, "adl_bloom_revision_read_plan")
        return gt, gbeg, ek, unc

    def close(self):
        if self._h:
            lib().adl_bloom_revision_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify(keys, key_begin, bitmaps, bitmap_off, offsets=None, bits_per_key: int = 10, stream=None):
    """Construction check (adl_bloom_verify): key i of host numpy `keys` belongs to the filter f with
    key_begin[f] <= i < key_begin[f+1] and is probed against bitmaps[bitmap_off[f]:bitmap_off[f+1]].
    Returns (keys the probe answers 0 for, index of the first one or None)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    kb = np.ascontiguousarray(key_begin, dtype=np.uint64)
    bo = np.ascontiguousarray(bitmap_off, dtype=np.uint64)
    bm = np.ascontiguousarray(bitmaps, dtype=np.uint8)
    if len(bo) != len(kb):
        raise ValueError("key_begin and bitmap_off need one entry per filter and one more")
    if offsets is None:
        n, stride, po = keys.shape[0], keys.shape[1], None
    else:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, stride, po = len(offsets) - 1, 0, offsets.ctypes.data
    missing, first = ctypes.c_uint64(), ctypes.c_uint64()
    kp = keys.ctypes.data if keys.size else np.zeros(16, np.uint8).ctypes.data
    bp = bm.ctypes.data if bm.size else np.zeros(16, np.uint8).ctypes.data
    _check(lib().adl_bloom_verify(kp, po, n, stride, kb.ctypes.data, len(kb) - 1, bp, bo.ctypes.data, bits_per_key,
                                  ctypes.byref(missing), ctypes.byref(first), _host_stream(stream)),
           "adl_bloom_verify")
    return missing.value, (None if missing.value == 0 else first.value)


# ------------------------------------------------------------------ synthetic inputs
def synth_keys16(n: int, seed: int = 0x5EED, skip: int = 0, device="cuda", stream=None):
    """SURVEY.md §8d SplitMix64 16-byte keys generated on the device: (n,16) uint8."""
    with _on(stream):
        keys = _torch().empty((max(n, 1), 16), dtype=_torch().uint8, device=device)
    _check(lib().adl_synth_keys16_device(_dptr(keys), seed, skip, n, _stream(stream)), "adl_synth_keys16_device")
    return keys[:n]


def synth_varlen(n: int, seed: int = 0x5EED, zipf_s: float = 1.1, device="cuda", stream=None):
    """Variable-length keys (8..256 B, Zipf lengths) on the device: (bytes, offsets[n+1] uint64)."""
    torch = _torch()
    # the prefix sum between the two launches is torch's: it runs on `stream` too
    with torch.cuda.stream(stream):
        lengths = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        _check(lib().adl_synth_varlen_lengths_device(_dptr(lengths), seed, n, zipf_s, _stream(stream)),
               "adl_synth_varlen_lengths_device")
        offs = torch.zeros(n + 1, dtype=torch.int64, device=device)
        if n:
            offs[1:] = torch.cumsum(lengths[:n].to(torch.int64), 0)
        total = int(offs[-1].item())
        data = torch.empty(((total + 15) // 16) * 16 + 16, dtype=torch.uint8, device=device)
        _check(lib().adl_synth_varlen_fill_device(_dptr(data), seed, total, _stream(stream)),
               "adl_synth_varlen_fill_device")
    return data, offs  # int64 storage, read as uint64 offsets by the C-ABI


def synth_probe_queries(n: int, seed: int = 0xFEED, q0: int = 0, num_tables: int = 256,
                        table_seed0: int = 0x5EED, keys_per_table: int = 1_000_000, device="cuda", stream=None):
    """Probe queries of BASELINE.json configs[4] on the device: (keys (n,16) u8, filter_id int32
    (read as uint32), member u8) -- see adl_synth_probe_queries_device."""
    torch = _torch()
    with _on(stream):
        keys = torch.empty((max(n, 1), 16), dtype=torch.uint8, device=device)
        fid = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        member = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    _check(lib().adl_synth_probe_queries_device(_dptr(keys), _dptr(fid), _dptr(member), seed, q0, n, num_tables,
                                                table_seed0, keys_per_table, _stream(stream)),
           "adl_synth_probe_queries_device")
    return keys[:n], fid[:n], member[:n]
