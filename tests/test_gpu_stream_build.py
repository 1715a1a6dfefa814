"""GPU: the streamed build (adl_bloom_stream, adlbloom.StreamBuilder): keys
appended in batches and hashed on arrival, filters built from the stored hash
pairs.  Expectations come from the CPU oracle (oracle.keys2block /
filter_block_final); at 3 M keys from adlbloom.build on the same keys, a path
the other tests pin to the oracle.  Shared inputs: tests/streamkeys.py.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import refcases as C
import streamkeys as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SKIP = 1  # ADL_BLOOM_SKIP_ADJACENT_DUPLICATES
ADL_ERR_WORKSPACE = -5


@pytest.fixture(scope="module")
def A():
    import torch

    import adlbloom

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return adlbloom


def _append_host(sb, ks, a, b, stream=None):
    d, o = K.part_absolute(ks, a, b)
    sb.append(d, o, stream=stream)


def _append_dev(sb, ks, a, b, keep, skew=None, stream=None):
    d, o = K.to_device(K.part(ks, a, b), skew=skew, keep=keep)
    keep.append((d, o))
    sb.append(d, o, stream=stream)


# ------------------------------------------------------------------ 1. split invariance
def _way_one(sb, ks, n, keep):
    _append_host(sb, ks, 0, n)


def _way_uneven(sb, ks, n, keep):
    rng = np.random.default_rng(13)
    cuts = np.sort(rng.integers(0, n + 1, size=12))
    cuts[3] = cuts[2]  # empty batches among them
    cuts[8] = cuts[7]
    edges = [0, *[int(c) for c in cuts], n]
    assert len(edges) == 14 and any(a == b for a, b in zip(edges, edges[1:]))
    for a, b in zip(edges, edges[1:]):
        _append_host(sb, ks, a, b)


def _way_key_by_key(sb, ks, n, keep):
    for i in range(70):
        _append_host(sb, ks, i, i + 1)
    _append_host(sb, ks, 70, n)


def _way_alternating(sb, ks, n, keep):
    edges = [0, 1, 600, 601, 1113, 2500, 4096, 6000, n]
    for j, (a, b) in enumerate(zip(edges, edges[1:])):
        if j % 2:
            _append_dev(sb, ks, a, b, keep)
        else:
            _append_host(sb, ks, a, b)


@pytest.mark.parametrize("way", [_way_one, _way_uneven, _way_key_by_key, _way_alternating],
                         ids=["one", "uneven13", "key_by_key", "host_device"])
@pytest.mark.parametrize("shape", ["k16", "var", "s24"])
def test_split_invariance(A, shape, way):
    """However a key sequence is cut into appends, the pair store is the same:
    read back through finishes at k = 6 and at k = 30, both equal the oracle's."""
    n = K.N_SPLIT
    ks = K.keyset(shape, n)
    keep = []
    sb = A.StreamBuilder()
    way(sb, ks, n, keep)
    assert list(sb.counts()) == [0, n]
    for bpk in (10, 44):
        K.assert_bitmaps(K.finished(sb, bpk), K.oracle_bitmaps(ks, [0, n], bpk, shape), f"{shape} bpk {bpk}")
    sb.close()


# ------------------------------------------------------------------ 2. run edges
def _edge_sizes(A):
    S = A.STREAM_RUN_KEYS
    return [0, 1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1]


def _edge_keyset(shape, n):
    """One batch of n keys.  var: empty keys first, in the middle and last, one key
    longer than a run's staged bytes (48 B per key of the run) and one of 70 001
    bytes (hashed from global memory: 64 KiB or more)."""
    key = ("edge", shape, n)
    if key not in K._cache:
        rng = np.random.default_rng(1000 + n)
        if shape == "var":
            lens = rng.integers(0, 70, size=n)
            if n:
                lens[0] = lens[n // 2] = lens[n - 1] = 0
            if n >= 63:
                lens[7] = 48 * 512 + 417
                lens[n - 3] = 70001
            K._cache[key] = K.from_lengths(lens, rng)
        else:
            stride = {"s24": 24, "s16": 16}[shape]
            K._cache[key] = (rng.integers(0, 256, size=(n, stride), dtype=np.uint8), None)
    return K._cache[key]


@pytest.mark.parametrize("place", ["host", "dev", "dev+1", "dev+9"])
@pytest.mark.parametrize("shape", ["var", "s24", "s16"])
def test_append_run_edges(A, shape, place):
    """Batches of 0, 1, 63..65, S-1..S+1 and 2S+1 keys (S: keys per run of the append
    kernel), one filter each, from host memory, from a 16-byte-aligned device
    buffer (whole-block reads) and from buffers 1 and 9 bytes off (exact reads)."""
    sizes = _edge_sizes(A)
    sb = A.StreamBuilder()
    keep = []
    want = []
    for n in sizes:
        ks = _edge_keyset(shape, n)
        if place == "host":
            sb.append(*K.part(ks, 0, n))
        else:
            skew = {"dev": 0, "dev+1": 1, "dev+9": 9}[place]
            d, o = K.to_device(ks, skew=skew, keep=keep)
            sb.append(d, o)
        sb.cut()
        want += K.oracle_bitmaps(ks, [0, n], 10, ("edge", shape, n))
    assert list(sb.counts()) == list(np.concatenate([[0], np.cumsum(sizes)]))
    K.assert_bitmaps(K.finished(sb, 10), want, f"{shape} {place}")
    sb.close()


# ------------------------------------------------------------------ 3. bits_per_key sweep
@pytest.mark.parametrize("n", [1, 2, 65, 50001])
def test_bits_per_key_sweep(A, n):
    """k = 1..30: the k = 6 pass A and the generic one, from one stream."""
    ks = K.keyset("k16", n, seed=3)
    sb = A.StreamBuilder()
    sb.append(ks[0])
    for bpk in (0, 1, 3, 9, 10, 11, 16, 30, 44, 50):
        K.assert_bitmaps(K.finished(sb, bpk), K.oracle_bitmaps(ks, [0, n], bpk, "sweep"), f"n {n} bpk {bpk}")
    sb.close()


@pytest.mark.parametrize("n", [0, 5583, 5584, 5585, 250001])
def test_chunk_edges(A, n):
    """Around pass A's keys per chunk, and several rounds of chunks."""
    ks = K.keyset("k16", n, seed=4)
    sb = A.StreamBuilder()
    sb.append(ks[0])
    sb.cut()
    assert list(sb.counts()) == [0, n]
    K.assert_bitmaps(K.finished(sb, 10), K.oracle_bitmaps(ks, [0, n], 10, "chunk"), f"n {n}")
    sb.close()


def _frame(bitmaps, kb, bpk):
    """Back-to-back bitmaps of the filters with bounds kb -> the filter block: i32 offsets[F],
    i32 offsets_start, i32 F, "bf:" + i32 bpk, i32 7."""
    import struct

    import adlbloom

    off = np.concatenate([[0], np.cumsum([adlbloom.bitmap_bytes(int(b - a), bpk) for a, b in zip(kb, kb[1:])])])
    assert int(off[-1]) == len(bitmaps)
    return (bytes(bitmaps) + b"".join(struct.pack("<i", int(o)) for o in off[:-1])
            + struct.pack("<ii", int(off[-1]), len(kb) - 1) + b"bf:" + struct.pack("<i", bpk) + struct.pack("<i", 7))


# ------------------------------------------------------------------ 4. cuts
LAYOUTS = {
    "empties": [0, 1, 0, 0, 6145, 0],
    "151x1": [1] * 151,
    "nine": [700, 0, 1, 64, 65, 1000, 513, 2, 300],  # more than the 8 whose descriptors ride in kernargs
}


@pytest.mark.parametrize("shape", ["k16", "var"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_cuts(A, oracle, layout, shape):
    sizes = LAYOUTS[layout]
    kb = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(kb[-1])
    ks = K.keyset(shape, n, seed=5)
    sb = A.StreamBuilder()
    keep = []
    for f, c in enumerate(sizes):
        a, b = int(kb[f]), int(kb[f + 1])
        if f % 2:
            _append_dev(sb, ks, a, b, keep)
        else:
            _append_host(sb, ks, a, b)
        if f + 1 < len(sizes) or c == 0:  # the last filter stays open unless it is empty
            sb.cut()
    assert list(sb.counts()) == list(kb)
    want = K.oracle_bitmaps(ks, kb, 10, (layout, shape))
    K.assert_bitmaps(K.finished(sb, 10), want, layout)
    # host bitmaps back to back (unaligned), as in a filter block
    exact = np.array([w.size for w in want], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(exact)]).astype(np.uint64)
    host = np.full(int(off[-1]) + 64, 0xA5, dtype=np.uint8)
    sb.finish_host(host[3:], off[:-1], 10)
    assert (host[:3] == 0xA5).all() and (host[3 + int(off[-1]):] == 0xA5).all()
    # the whole block: those bitmaps framed from the stream's own counts, as
    # FilterBlockWriter::Final frames them (src/filter_block.cpp:77-102)
    assert _frame(host[3:3 + int(off[-1])], sb.counts(), 10) == oracle.filter_block_final([bytes(w) for w in want], 10)
    sb.close()


# ------------------------------------------------------------------ 5. adjacent duplicates
def _dup_keys(shape):
    """Runs of 1-5 equal keys (equal empty keys among the var-len ones)."""
    key = ("dups", shape)
    if key not in K._cache:
        rng = np.random.default_rng(55)
        runs = rng.integers(1, 6, size=420)
        if shape == "k16":
            base = K.keyset("k16", len(runs), seed=6)[0]
            K._cache[key] = (np.ascontiguousarray(np.repeat(base, runs, axis=0)), None)
        else:
            uniq = [bytes(rng.integers(0, 256, size=int(l), dtype=np.uint8)) for l in rng.integers(0, 40, size=len(runs))]
            uniq[0] = uniq[200] = uniq[201] = b""  # (two runs of empty keys in a row: one longer run)
            K._cache[key] = K.from_list([k for k, r in zip(uniq, runs) for _ in range(int(r))])
    return K._cache[key]


@pytest.mark.parametrize("bpk", [3, 10])
@pytest.mark.parametrize("flags", [0, SKIP])
@pytest.mark.parametrize("shape", ["k16", "var"])
def test_adjacent_duplicates(A, shape, flags, bpk):
    """Equal keys in a row, across batch boundaries and across a cut: the same
    bitmaps with and without the skip (m counts every key)."""
    ks = _dup_keys(shape)
    n = K.count(ks)
    eq = [i for i in range(1, n) if K.part(ks, i, i + 1)[0].tobytes() == K.part(ks, i - 1, i)[0].tobytes()
          and (ks[1] is None or ks[1][i + 1] - ks[1][i] == ks[1][i] - ks[1][i - 1])]
    assert len(eq) > n // 3
    cut_at = eq[len(eq) // 2]          # a cut between two equal keys
    edges = sorted({0, eq[3], eq[10], cut_at, eq[-5], n})  # batch boundaries inside runs
    sb = A.StreamBuilder()
    keep = []
    for j, (a, b) in enumerate(zip(edges, edges[1:])):
        if a == cut_at:
            sb.cut()
        if j % 2:
            _append_dev(sb, ks, a, b, keep)
        else:
            _append_host(sb, ks, a, b)
    kb = [0, cut_at, n]
    assert list(sb.counts()) == kb
    K.assert_bitmaps(K.finished(sb, bpk, flags=flags), K.oracle_bitmaps(ks, kb, bpk, ("dups", shape)),
                     f"{shape} flags {flags} bpk {bpk}")
    sb.close()


# ------------------------------------------------------------------ 6. growth
@pytest.mark.parametrize("reserve", [0, 1000])
def test_growth_reset_and_refinish(A, reserve):
    """200 000 keys in 40 appends with nothing waited for in between: the store
    regrows several times with appends in flight.  Then reset and another key
    set; and the same pairs finished twice."""
    n = 200_000
    ks = K.keyset("k16", n, seed=7)
    sb = A.StreamBuilder(reserve_keys=reserve)
    keep = []
    step = n // 40
    for j in range(40):
        a, b = j * step, (j + 1) * step
        if j % 3 == 2:
            _append_dev(sb, ks, a, b, keep)
        else:
            _append_host(sb, ks, a, b)
    K.assert_bitmaps(K.finished(sb, 10), K.oracle_bitmaps(ks, [0, n], 10, "grow"), "first")
    sb.reset()
    assert list(sb.counts()) == [0]
    ks2 = K.keyset("var", 30_000, seed=8)
    _append_host(sb, ks2, 0, 12_345)
    _append_host(sb, ks2, 12_345, 30_000)
    K.assert_bitmaps(K.finished(sb, 10), K.oracle_bitmaps(ks2, [0, 30_000], 10, "grow2"), "after reset, bpk 10")
    K.assert_bitmaps(K.finished(sb, 3), K.oracle_bitmaps(ks2, [0, 30_000], 3, "grow2"), "after reset, bpk 3")
    sb.close()


# ------------------------------------------------------------------ 7. several pass-A rounds
def test_three_million_device_keys(A):
    import torch

    n = 3_000_000
    keys = A.synth_keys16(n, seed=0x57EA)
    edges = [0, 1, 400_001, 400_002, 1_300_000, 2_000_003, 2_999_999, n]
    sb = A.StreamBuilder(reserve_keys=n)
    for a, b in zip(edges, edges[1:]):
        sb.append(keys[a:b])
    out, boff, sizes = sb.finish(10)
    want = A.build(keys, bits_per_key=10)
    torch.cuda.synchronize()
    assert int(sizes[0]) == want.numel()
    assert torch.equal(out[:int(sizes[0])], want)
    sb.close()


# ------------------------------------------------------------------ 8. stream order
def test_stream_order(A):
    """Appends on one non-blocking stream behind a delay, the finish on another:
    the finish waits for the appends (their inputs arrive late, over decoys),
    nothing waits for the host, and the host batch is copied before the append
    returns."""
    import torch

    import streamorder as SO

    n_dev, n_host = 3000, 2500
    ks = K.keyset("k16", n_dev + n_host, seed=9)
    decoy = K.keyset("k16", n_dev, seed=10)[0]
    true_dev = ks[0][:n_dev]
    host_keys = np.array(ks[0][n_dev:])
    n = n_dev + n_host
    case = SO.Case()
    d_keys = case.input(true_dev, decoy).reshape(n_dev, 16)
    alloc = A.bitmap_alloc_bytes(n, 10)
    out = case.output(alloc)
    ws_bytes = A.workspace_bytes([n], 10)
    ws = case.workspace(ws_bytes)
    s2 = torch.cuda.Stream()
    with torch.cuda.stream(s2):  # (a stream's first submission sets up its hardware queue, which takes milliseconds)
        torch.zeros(16, dtype=torch.uint8, device="cuda").fill_(1)
    s2.synchronize()
    sb = A.StreamBuilder()
    boff = np.zeros(1, dtype=np.uint64)
    early = {}

    def entry(s):
        probe = torch.cuda.Event()
        sb.append(d_keys, stream=s)
        sb.append(host_keys, stream=s)
        probe.record(s)
        early["append"] = not probe.query()  # the host append came back with its work still queued
        host_keys[:] = 0xEE                  # its buffer is the caller's again
        A._check(A.lib().adl_bloom_stream_finish_device(sb._h, 10, 0, out.data_ptr(), boff.ctypes.data, ws.data_ptr(),
                                                        ws_bytes, SO.sptr(s2)), "finish")
        done = torch.cuda.Event()
        done.record(s2)
        s.wait_event(done)  # the consumer reads behind the finish's stream

    case.run(entry)
    s2.synchronize()
    assert case.returned_early and early["append"]
    SO.check(case.result(out, A.bitmap_bytes(n, 10)), K.oracle_bitmaps(ks, [0, n], 10, "order")[0], "bitmap")
    sb.close()
    SO.release_delay()


# ------------------------------------------------------------------ 9. buffer contracts
def test_buffer_contracts(A):
    """Outputs and workspace at exactly the promised sizes inside guard bands;
    a workspace one byte short is refused with nothing written."""
    import torch

    from guardband import Guarded, check_all

    sizes = [700, 0, 1, 64, 65, 1000, 513, 2, 300, 5000]
    kb = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(kb[-1])
    ks = K.keyset("var", n, seed=11)
    sb = A.StreamBuilder()
    for f in range(len(sizes)):
        _append_host(sb, ks, int(kb[f]), int(kb[f + 1]))
        sb.cut()
    alloc = np.array([A.bitmap_alloc_bytes(c, 10) for c in sizes], dtype=np.uint64)
    boff = np.concatenate([[0], np.cumsum(alloc)[:-1]]).astype(np.uint64)
    ws_bytes = sb.workspace_bytes(10)
    assert ws_bytes == A.workspace_bytes(sizes, 10)
    out = Guarded(int(alloc.sum()), 16, name="bitmaps")
    ws = Guarded(ws_bytes, 256, name="workspace")
    L = A.lib()
    st = A._stream(None)
    rc = L.adl_bloom_stream_finish_device(sb._h, 10, 0, out.ptr, boff.ctypes.data, ws.ptr, ws_bytes - 1, st)
    torch.cuda.synchronize()
    assert rc == ADL_ERR_WORKSPACE
    assert bool((out.view == 0xA5).all()) and bool((ws.view == 0xA5).all())
    A._check(L.adl_bloom_stream_finish_device(sb._h, 10, 0, out.ptr, boff.ctypes.data, ws.ptr, ws_bytes, st), "finish")
    torch.cuda.synchronize()
    check_all(out, ws)
    h = out.numpy()
    want = K.oracle_bitmaps(ks, kb, 10, "contracts")
    K.assert_bitmaps([h[int(o):int(o) + w.size] for o, w in zip(boff, want)], want, "guarded")
    # host bitmaps at exactly n*bpk+7 bytes each, back to back, inside bands
    exact = np.array([w.size for w in want], dtype=np.uint64)
    hoff = np.concatenate([[0], np.cumsum(exact)]).astype(np.uint64)
    hb = Guarded(int(hoff[-1]), 1, pinned_host=True, skew=5, name="host bitmaps")
    A._check(L.adl_bloom_stream_finish(sb._h, 10, 0, hb.ptr, hoff.ctypes.data, None), "finish host")
    hb.check()
    hv = hb.view.numpy()
    K.assert_bitmaps([hv[int(o):int(o) + w.size] for o, w in zip(hoff, want)], want, "guarded host")
    sb.close()


# ------------------------------------------------------------------ 10. write-through
WT_SIZES = [700, 0, 1, 64, 65, 1000, 513, 2, 300, 5000]  # ten filters: the pack path and the FilterTable


def _wt_stream(A, shape, sizes, keep):
    kb = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ks = K.keyset(shape, int(kb[-1]), seed=31)
    sb = A.StreamBuilder()
    for f in range(len(sizes)):
        a, b = int(kb[f]), int(kb[f + 1])
        if f % 2:
            _append_dev(sb, ks, a, b, keep)
        else:
            _append_host(sb, ks, a, b)
        sb.cut()
    return sb, ks, kb


@pytest.mark.parametrize("verify", [False, True], ids=["plain", "verify"])
@pytest.mark.parametrize("sizes", [[6145], WT_SIZES], ids=["one_filter", "ten_filters"])
@pytest.mark.parametrize("shape", ["k16", "var"])
def test_cache_build_stream(A, oracle, shape, sizes, verify):
    """FilterCache.build_stream: the block FilterCache.build gives for the same keys (and the oracle's),
    resident after publish -- a multi-get over the table is the oracle's -- and given back by abandon."""
    keep = []
    sb, ks, kb = _wt_stream(A, shape, sizes, keep)
    flags = A.CACHE_VERIFY if verify else 0
    want = oracle.filter_block_final([bytes(w) for w in K.oracle_bitmaps(ks, kb, 10, ("wt", shape, len(sizes)))], 10)
    ref_cache = A.FilterCache(8 << 20, max_tables=8)
    ref_block, rt = ref_cache.build(ks[0], kb, offsets=ks[1], bits_per_key=10, flags=flags)
    ref_cache.abandon(rt)
    ref_cache.close()
    cache = A.FilterCache(8 << 20, max_tables=8)
    tables0, used0 = cache.stats()
    block, t = cache.build_stream(sb, 10, flags=flags)
    assert block == ref_block == want
    oid = b"streamed-table"
    assert oid not in cache and cache.stats()[0] == tables0 and cache.stats()[1] > used0
    used1 = cache.stats()[1]
    cache.publish(t, oid)
    assert oid in cache and cache.stats() == (tables0 + 1, used1)
    # every filter of the resident block: its own keys, and keys it does not hold
    n = int(kb[-1])
    absent = K.keyset(shape, 2000, seed=32)
    for f in range(len(sizes)):
        a, b = int(kb[f]), int(kb[f + 1])
        bm = K.oracle_bitmaps(ks, kb, 10, ("wt", shape, len(sizes)))[f]
        for qs in (K.part(ks, a, min(b, a + 1500)), absent):
            if K.count(qs) == 0:
                continue
            got, unc = cache.probe([oid], np.zeros(K.count(qs), np.uint32), qs[0], offsets=qs[1], filter=f)
            if qs[1] is None:
                exp = oracle.probe(qs[0], bm, bits_per_key=10)
            else:
                exp = oracle.probe(qs[0], bm, offsets=qs[1], bits_per_key=10)
            assert unc == 0 and np.array_equal(got, exp), (f, n)
    # the stream is not consumed: a second build, abandoned, gives its bytes back
    block2, t2 = cache.build_stream(sb, 10, flags=flags)
    assert block2 == want and cache.stats()[1] > used1
    cache.abandon(t2)
    assert cache.stats() == (tables0 + 1, used1)
    assert cache.remove(oid) and cache.stats() == (tables0, used0)
    cache.close()
    sb.close()


def test_cache_build_stream_verify_failure(A):
    """A corrupted bitmap (ADL_TEST_FAULT_CACHE_BUILD_CORRUPT) fails the verify from the pairs: no
    ticket, nothing resident, the range given back; without verify the same fault goes unnoticed."""
    keep = []
    sb, ks, kb = _wt_stream(A, "var", WT_SIZES, keep)
    cache = A.FilterCache(8 << 20, max_tables=8)
    stats0 = cache.stats()
    A.test_fault(A.TEST_FAULT_CACHE_BUILD_CORRUPT, 0)
    rc, block, t = cache.build_stream_status(sb, 10, flags=A.CACHE_VERIFY)
    assert rc == A.ADL_FILTER_BLOCK_ERROR and block is None and t is None
    assert cache.stats() == stats0
    rc, block, t = cache.build_stream_status(sb, 10, flags=A.CACHE_VERIFY)  # the fault fired once
    assert rc == 0
    cache.abandon(t)
    assert cache.stats() == stats0
    cache.close()
    sb.close()


def test_cache_build_stream_refusals(A):
    import ctypes

    L = A.lib()
    sb = A.StreamBuilder()
    sb.append(K.keyset("k16", 100, seed=33)[0])
    cache = A.FilterCache(1 << 20, max_tables=4)
    buf = np.zeros(4096, np.uint8)
    h, got = ctypes.c_void_p(), ctypes.c_uint64()
    args = lambda c, s, bpk, flags, p, cap: L.adl_bloom_filter_cache_build_stream(  # noqa: E731
        c, s, bpk, flags, p, cap, ctypes.byref(got), ctypes.byref(h), None)
    assert args(None, sb._h, 10, 0, buf.ctypes.data, 4096) == -1
    assert args(cache._h, None, 10, 0, buf.ctypes.data, 4096) == -1
    assert args(cache._h, sb._h, -1, 0, buf.ctypes.data, 4096) == -1
    assert args(cache._h, sb._h, 10, 0x80, buf.ctypes.data, 4096) == -1
    assert args(cache._h, sb._h, 10, 0, None, 4096) == -1
    assert args(cache._h, sb._h, 10, 0, buf.ctypes.data, 16) == -1 and got.value == A.filter_block_bytes([0, 100], 10)
    assert cache.stats() == (0, 0)
    cache.close()
    sb.close()


# ------------------------------------------------------------------ 12. the C++ mirror
def _run(exe, args, env_extra, tmp=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ADL_BLOOM_STREAM")}
    env.update(env_extra)
    r = subprocess.run([os.path.join(ROOT, "adlsm-tree_amd", "bin", exe), *args], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (exe, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.parametrize("batch_keys", [None, 1000, 37])
def test_cpp_mirror_streaming(golden, batch_keys):
    """FilterBlockWriter / SSTableWriter with the streamed build (stream_build_test.cpp): blocks
    and files byte-identical to the ordinary writer's inside the binary; here the reference's
    block hash and oid, at the default flush size and at small ones."""
    out = _run("stream_build_test", [], {} if batch_keys is None else {"ADL_BLOOM_STREAM_BATCH_KEYS": str(batch_keys)})
    lines = dict((l.split()[0] + (l.split()[1] if l.startswith("table") else ""), l.split()) for l in out.splitlines()
                 if l.startswith(("block", "table")))
    fb = golden["appendix_b"]["filter_block_test"]
    assert lines["block"][1] == fb["sha256"] and int(lines["block"][2]) == fb["bytes"]
    st = golden["appendix_b"]["sstable_test"]
    assert lines["table1"][2] == st["oid"] and int(lines["table1"][3]) == st["bytes"]
    assert "all checks passed" in out


def test_cpp_mirror_env_switch(golden, tmp_path):
    """ADL_BLOOM_STREAM_BUILD=1 turns the streamed build on for the mirror classes: the existing
    test binaries give the reference's block and file."""
    import hashlib

    env = {"ADL_BLOOM_STREAM_BUILD": "1", "ADL_BLOOM_STREAM_BATCH_KEYS": "4096"}
    blk = tmp_path / "block.bin"
    _run("filter_block_test", [str(blk)], env)
    assert hashlib.sha256(blk.read_bytes()).hexdigest() == golden["appendix_b"]["filter_block_test"]["sha256"]
    for mode in ([], ["batch"]):
        oid, size, _ = _run("sstable_test", [*mode, "1", str(tmp_path)], env).split()
        assert oid == golden["appendix_b"]["sstable_test"]["oid"]
        assert int(size) == golden["appendix_b"]["sstable_test"]["bytes"]
        assert hashlib.sha256((tmp_path / f"{oid}.sst").read_bytes()).hexdigest() == oid


# ------------------------------------------------------------------ 13. reference fixtures
@pytest.mark.parametrize("name", list(C.BLOCKS))
def test_reference_fixture_blocks(A, name):
    """The recorded blocks of the reference's FilterBlockWriter (tests/golden/filter_block_ref.json,
    cases from tests/refcases.py), without the oracle: the streamed bitmaps back to back, framed as
    FilterBlockWriter::Final frames them (src/filter_block.cpp:77-102), have the recorded length and SHA-256."""
    rec = C.load_json()["blocks"][name]
    shape, bpk, counts = C.BLOCKS[name]
    k = C.block_keys(name)
    assert k.sha() == rec["keys_sha256"]
    ks = (np.ascontiguousarray(k.fixed(16)), None) if shape == "split16" else (k.data, k.offs.view(np.uint64))
    kb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    sb = A.StreamBuilder()
    keep = []
    for f in range(len(counts)):
        a, b = int(kb[f]), int(kb[f + 1])
        mid = (a + b) // 2  # two appends per filter, one from host and one from device memory
        _append_host(sb, ks, a, mid)
        _append_dev(sb, ks, mid, b, keep)
        sb.cut()
    assert list(sb.counts()) == list(kb)
    sizes = [A.bitmap_bytes(int(c), bpk) for c in counts]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    buf = np.zeros(int(off[-1]), dtype=np.uint8)
    sb.finish_host(buf, off[:-1], bpk)
    block = _frame(buf, kb, bpk)
    assert len(block) == rec["bytes"]
    assert C.sha(block) == rec["sha256"]
    sb.close()


# ------------------------------------------------------------------ 11. threads
def test_threads(A):
    """Two threads stream into their own objects while a third runs ordinary builds."""
    import torch

    n = 40_000
    sets = {"a": K.keyset("k16", n, seed=21), "b": K.keyset("var", n, seed=22), "c": K.keyset("k16", n, seed=23)}
    got, errors = {}, []

    def streamer(name):
        try:
            torch.cuda.set_device(0)
            st = torch.cuda.Stream()
            ks = sets[name]
            res = []
            for _ in range(3):
                sb = A.StreamBuilder()
                keep = []
                for j in range(16):
                    a, b = j * n // 16, (j + 1) * n // 16
                    if j % 2:
                        _append_dev(sb, ks, a, b, keep, stream=st)
                    else:
                        _append_host(sb, ks, a, b, stream=st)
                res.append(K.finished(sb, 10, stream=st)[0].copy())
                sb.close()
            got[name] = res
        except Exception as e:  # noqa: BLE001
            errors.append((name, e))

    def builder():
        try:
            torch.cuda.set_device(0)
            st = torch.cuda.Stream()
            d = torch.from_numpy(np.array(sets["c"][0])).cuda()
            res = []
            for _ in range(6):
                bm = A.build(d, bits_per_key=10, stream=st)
                st.synchronize()
                res.append(bm.cpu().numpy())
            got["c"] = res
        except Exception as e:  # noqa: BLE001
            errors.append(("c", e))

    threads = [threading.Thread(target=streamer, args=("a",)), threading.Thread(target=streamer, args=("b",)),
               threading.Thread(target=builder)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for name, ks in sets.items():
        want = K.oracle_bitmaps(ks, [0, n], 10, ("threads", name))
        for r in got[name]:
            K.assert_bitmaps([r], want, name)
