"""GPU: stream ordering of the C-ABI's entry points on non-default streams
(the harness and its reasoning: tests/streamorder.py).

include/adl_bloom.h: work is enqueued on the caller's stream; the *_device
functions do not synchronise; the host-pointer functions return with their
results in host memory, and for them stream == NULL is a non-blocking stream
of the calling thread.  Every other GPU test runs on torch's default stream,
handle 0, where a launch, memset or copy on the wrong stream cannot show.

Shapes are the smallest that still reach every launch of their path:

  build_device         20 011 x 16 B keys at bpk 10 (bin16 dense, descriptors in
                       the kernarg) and bpk 3 (generic pass A); 5 000 keys of
                       0..90 B (hashing pass, SrcH pass A, pass B); 100 000 x
                       16 B keys with ADL_BLOOM_BUILD_QUEUES=3 (256 chunks, a
                       multiple of 8, so both passes queue and the counters'
                       hipMemsetAsync is enqueued: the launch line is asserted)
  build_segmented_device_ex
                       10 filters (more than 8: UploadRing upload and
                       fill_maps_kernel), flags 0 and SKIP_ADJACENT_DUPLICATES;
                       the host key_begin / bitmap_off arrays are overwritten
                       (with zeros: a late read could not index out of range)
                       as soon as the call has returned
  filter_block_build_device
                       70 filters of 0..300 keys (two pack launches at 64
                       filters each), and no filter at all (19 bytes)
  build then probe     build_device followed on the same stream, with no
                       synchronise, by probe / probe_multi / probe_ranges /
                       probe_fanout / verify: 5 000 queries, half inserted
  probe_batch_device   2^20 + 777 queries over 8 filters of 30 000 keys: the
                       nine-kernel binned pipeline
  murmur3 / synth_*    n = 4 096

Every *_device case first runs once on the null stream, synchronised (code
objects loaded, hipFuncSetAttribute done), and then asserts that the entry
point returned while the delay was still running.  None of them was found to
block.  (A fifth build of more than 8 filters between synchronisations would:
UploadRing::upload waits for its slot by design.  No case makes more than
four per thread.)

The host-pointer entry points run with stream = a stream that carries the
delay and with stream = None; their outputs are compared at return.  The host
pipeline splits by key bytes (about 128 MB a group), not by filter count: the
cases set ADL_BLOOM_PIPE_MB=1, and 10 filters of 20 000 x 16 B keys then make
four groups (both buffer parities reused).

adl_bloom_build_positions: the table layout comes from the workspace it is
given, whatever the calling thread has built since in another workspace
(claim then dense and dense then claim), and the readback runs on the stream
the *_device build with the same `stream` argument ran on, NULL being the
null stream (a build behind the delay, then positions with no synchronise).

The adlbloom wrappers that take `stream` are run on a delayed stream that is
not the current one (the last section): they order their own torch work and
their temporaries' lifetimes against that stream.
"""
import threading

import numpy as np
import pytest

import streamorder as so

pytestmark = pytest.mark.gpu

SKIP_DUP = 1


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield torch
    so.release_delay()


@pytest.fixture(scope="module")
def ab():
    import adlbloom

    adlbloom.lib()
    return adlbloom


def ok(rc, what):
    assert rc == 0, (what, rc)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def kb_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def drive(setup):
    """setup(case) -> (entry(stream), verify(case)).  Warm the entry up on the null
    stream with buffers of its own, then run it through the harness, require
    that it did not wait for the stream, and compare."""
    import torch

    warm = so.Case()
    entry, _ = setup(warm)
    entry(None)
    torch.cuda.synchronize()
    case = so.Case()
    entry, verify = setup(case)
    case.run(entry)
    assert case.returned_early, "the entry point came back only after the delay: it waits for the stream"
    verify(case)
    del warm


# ---------------------------------------------------------------- shared inputs (computed once, never modified)
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def keys16(oracle, seed, n):
    return memo(("k16", seed, n), lambda: oracle.splitmix_keys16(seed, n))


def varlen_sets(n):
    """(data, offsets) true and decoy: n keys of 0..90 bytes; the decoy has the
    lengths in reverse order (the same total) and other bytes."""
    def make():
        rng = np.random.default_rng(90)
        lens = rng.integers(0, 91, n)
        lens[:3] = (0, 90, 1)
        total = int(lens.sum())
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        doffs = np.concatenate([[0], np.cumsum(lens[::-1])]).astype(np.uint64)
        data = rng.integers(0, 256, total, dtype=np.uint8)
        ddata = rng.integers(0, 256, total, dtype=np.uint8)
        return data, offs, ddata, doffs
    return memo(("var", n), make)


# ---------------------------------------------------------------- the control
def test_control_copy_on_another_stream_is_caught(dev):
    """A fake entry point that copies its input to its output on a second
    stream instead of the one it was given: the copy runs before the producer
    (it reads the decoy) and the producer's 0xA5 lands on top of it.  The
    comparison reports it; the same copy on the given stream passes."""
    true = np.arange(1 << 16, dtype=np.uint32)
    decoy = true[::-1].copy()
    other = dev.cuda.Stream()

    def run(on_other):
        case = so.Case()
        src = case.input(true, decoy)
        out = case.output(true.nbytes)

        def entry(s):
            with dev.cuda.stream(other if on_other else s):
                out.copy_(src)

        case.run(entry)
        other.synchronize()
        assert case.returned_early
        so.check(case.result(out), true, "copy")

    run(False)
    with pytest.raises(so.StreamOrderError) as e:
        run(True)
    assert e.value.count > 0


# ---------------------------------------------------------------- adl_bloom_build_device
def build_setup(ab, oracle, n, bpk, true, decoy, offs=None):
    """offs: (true offsets, decoy offsets) of variable-length keys"""
    L = ab.lib()
    nbytes, alloc = ab.bitmap_bytes(n, bpk), ab.bitmap_alloc_bytes(n, bpk)
    wsb = ab.workspace_bytes([n], bpk)
    want = oracle.keys2block(true, None if offs is None else offs[0], bits_per_key=bpk)

    def setup(case):
        keys = case.input(true, decoy, pad=32)
        d_offs = None if offs is None else case.input(offs[0], offs[1])
        bm, ws = case.output(alloc), case.workspace(wsb)

        def entry(s):
            ok(L.adl_bloom_build_device(keys.data_ptr(), None if d_offs is None else d_offs.data_ptr(), n,
                                        0 if offs is not None else 16, bpk, bm.data_ptr(), ws.data_ptr(), wsb,
                                        so.sptr(s)), "adl_bloom_build_device")

        def verify(c):
            got = c.result(bm)
            so.check(got[:nbytes], want, "bitmap")
            assert not got[nbytes:alloc].any(), "the pad bytes are written as zero"

        return entry, verify

    return setup


@pytest.mark.parametrize("bpk", [10, 3], ids=["bpk10-bin16", "bpk3-generic"])
def test_build_device_16b(dev, ab, oracle, bpk):
    n = 20_011
    drive(build_setup(ab, oracle, n, bpk, keys16(oracle, 1, n), keys16(oracle, 2, n)))


def test_build_device_varlen(dev, ab, oracle):
    n = 5_000
    data, offs, ddata, doffs = varlen_sets(n)
    drive(build_setup(ab, oracle, n, 10, data, ddata, (offs, doffs)))


def test_build_device_queued(dev, ab, oracle, knobs, capfd):
    knobs.set("ADL_BLOOM_BUILD_QUEUES", "3")
    knobs.set("ADL_BLOOM_DEBUG", "1")
    n = 100_000
    capfd.readouterr()
    drive(build_setup(ab, oracle, n, 10, keys16(oracle, 3, n), keys16(oracle, 4, n)))
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "adl_bloom launch:" in ln]
    assert len(lines) == 2 and all("pass A queued" in ln and "pass B queued" in ln for ln in lines), lines


# ---------------------------------------------------------------- adl_bloom_build_segmented_device_ex
SEG_SIZES = [0, 1, 6145, 300, 7, 2, 4097, 12, 1000, 5]


def with_repeats(keys):
    """every fifth key repeats the one before it (versions of one user key in a row)"""
    keys = keys.copy()
    keys[4::5] = keys[3::5][:len(keys[4::5])]
    return keys


@pytest.mark.parametrize("flags", [0, SKIP_DUP], ids=["flags0", "skip-adjacent-duplicates"])
def test_build_segmented_device_ex(dev, ab, oracle, flags):
    L = ab.lib()
    kb = kb_of(SEG_SIZES)
    n, F, bpk = int(kb[-1]), len(SEG_SIZES), 10
    true, decoy = with_repeats(keys16(oracle, 11, n)), with_repeats(keys16(oracle, 12, n))
    sizes = [ab.bitmap_bytes(c, bpk) for c in SEG_SIZES]
    alloc = [ab.bitmap_alloc_bytes(c, bpk) for c in SEG_SIZES]
    boff = kb_of(alloc)[:-1].copy()
    wsb = ab.workspace_bytes(SEG_SIZES, bpk)
    want = np.zeros(sum(alloc), np.uint8)
    for f in range(F):
        want[int(boff[f]):int(boff[f]) + sizes[f]] = oracle.keys2block(true[int(kb[f]):int(kb[f + 1])])

    def setup(case):
        keys = case.input(true, decoy, pad=32)
        out, ws = case.output(sum(alloc)), case.workspace(wsb)

        def entry(s):
            h_kb, h_boff = kb.copy(), boff.copy()
            ok(L.adl_bloom_build_segmented_device_ex(keys.data_ptr(), None, 16, h_kb.ctypes.data, F, bpk,
                                                     out.data_ptr(), h_boff.ctypes.data, flags, ws.data_ptr(), wsb,
                                                     so.sptr(s)), "adl_bloom_build_segmented_device_ex")
            # the library has consumed the host arrays by now; the build has not run yet
            h_kb[:] = 0
            h_boff[:] = 0

        return entry, lambda c: so.check(c.result(out), want, "bitmaps")

    drive(setup)


# ---------------------------------------------------------------- adl_bloom_filter_block_build_device
@pytest.mark.parametrize("F", [70, 0], ids=["70-filters", "no-filter"])
def test_filter_block_build_device(dev, ab, oracle, F):
    L = ab.lib()
    bpk = 10
    rng = np.random.default_rng(70)
    counts = rng.integers(0, 301, F)
    if F:
        counts[:3] = (0, 300, 1)
    kb = kb_of(counts)
    n = int(kb[-1])
    true, decoy = keys16(oracle, 21, max(n, 1)), keys16(oracle, 22, max(n, 1))
    want = np.frombuffer(oracle.filter_block_final(
        [oracle.keys2block(true[int(kb[f]):int(kb[f + 1])]).tobytes() for f in range(F)], bpk), dtype=np.uint8)
    nbytes = L.adl_bloom_filter_block_bytes(kb.ctypes.data, F, bpk)
    wsb = L.adl_bloom_filter_block_workspace_bytes(kb.ctypes.data, F, bpk)
    assert nbytes == want.size and wsb > 0
    if F == 0:
        assert nbytes == 19

    def setup(case):
        keys = case.input(true, decoy, pad=32)
        block, ws = case.output(nbytes), case.workspace(wsb)

        def entry(s):
            h_kb = kb.copy()
            ok(L.adl_bloom_filter_block_build_device(keys.data_ptr(), None, 16, h_kb.ctypes.data, F, bpk,
                                                     block.data_ptr(), nbytes, ws.data_ptr(), wsb, so.sptr(s)),
               "adl_bloom_filter_block_build_device")
            h_kb[:] = 0

        return entry, lambda c: so.check(c.result(block, nbytes), want, "filter block")

    drive(setup)


# ---------------------------------------------------------------- build, then probe, one stream, no synchronise
@pytest.mark.parametrize("which", ["probe", "probe_multi", "probe_ranges", "probe_fanout", "verify"])
def test_build_then_probe(dev, ab, oracle, which):
    L = ab.lib()
    n, bpk, nq = 20_011, 10, 5_000
    true, decoy = keys16(oracle, 1, n), keys16(oracle, 2, n)
    nbytes, alloc = ab.bitmap_bytes(n, bpk), ab.bitmap_alloc_bytes(n, bpk)
    wsb = ab.workspace_bytes([n], bpk)
    bm_want = memo(("bm", 1, n, bpk), lambda: oracle.keys2block(true, bits_per_key=bpk))
    q = np.concatenate([true[:nq // 2], keys16(oracle, 99, nq - nq // 2)])  # half inserted, half fresh
    dq = np.ascontiguousarray(q[::-1])
    ans = memo(("ans", 1, n, bpk), lambda: oracle.probe(q, bm_want, bits_per_key=bpk))
    assert ans[:nq // 2].all() and not ans.all()
    # fan-out: the first 100 keys ask filter 0 twice, filter 1 (past the last: 0) once
    per = np.where(np.arange(nq) < 100, 3, 1)
    pb = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    pf = np.zeros(int(pb[-1]), np.uint32)
    pf[pb[:100] + 2] = 1
    fan_want = np.repeat(ans, per)
    fan_want[pb[:100] + 2] = 0

    def setup(case):
        keys = case.input(true, decoy, pad=32)
        qs = case.input(q, dq, pad=32)
        bm, ws = case.output(alloc), case.workspace(wsb)
        fid = case.const(np.zeros(nq, np.uint32))
        off2 = case.const(u64([0, nbytes]))
        end1 = case.const(u64([nbytes]))
        kbeg = case.const(u64([0, n]))
        d_pb, d_pf = case.const(pb), case.const(pf)
        out = case.output({"probe_fanout": pf.size, "verify": 16}.get(which, nq))
        st = so.sptr

        def entry(s):
            ok(L.adl_bloom_build_device(keys.data_ptr(), None, n, 16, bpk, bm.data_ptr(), ws.data_ptr(), wsb, st(s)),
               "adl_bloom_build_device")
            if which == "probe":
                rc = L.adl_bloom_probe_device(qs.data_ptr(), None, nq, 16, bpk, bm.data_ptr(), nbytes, out.data_ptr(),
                                              st(s))
            elif which == "probe_multi":
                rc = L.adl_bloom_probe_multi_device(qs.data_ptr(), None, nq, 16, fid.data_ptr(), 1, bm.data_ptr(),
                                                    off2.data_ptr(), bpk, out.data_ptr(), st(s))
            elif which == "probe_ranges":
                rc = L.adl_bloom_probe_ranges_device(qs.data_ptr(), None, nq, 16, fid.data_ptr(), 1, bm.data_ptr(),
                                                     off2.data_ptr(), end1.data_ptr(), bpk, out.data_ptr(), st(s))
            elif which == "probe_fanout":
                rc = L.adl_bloom_probe_fanout_device(qs.data_ptr(), None, nq, 16, d_pb.data_ptr(), d_pf.data_ptr(),
                                                     pf.size, 1, bm.data_ptr(), off2.data_ptr(), None, bpk,
                                                     out.data_ptr(), st(s))
            else:  # every build key against the filter it went into
                rc = L.adl_bloom_verify_device(keys.data_ptr(), None, n, 16, kbeg.data_ptr(), 1, bm.data_ptr(),
                                               off2.data_ptr(), None, bpk, out.data_ptr(), st(s))
            ok(rc, which)

        def verify(c):
            so.check(c.result(bm, nbytes), bm_want, "bitmap")
            if which == "verify":
                so.check(c.result(out, 16), np.array([0, 2**64 - 1], np.uint64), "d_result")
            elif which == "probe_fanout":
                so.check(c.result(out, pf.size), fan_want, "answers")
            else:
                so.check(c.result(out, nq), ans, "answers")

        return entry, verify

    drive(setup)


# ---------------------------------------------------------------- adl_bloom_probe_batch_device
def test_probe_batch_device_binned(dev, ab, oracle):
    L = ab.lib()
    T, per, bpk = 8, 30_000, 10
    n = (1 << 20) + 777

    def arena(seed0):
        bms = [oracle.keys2block(oracle.splitmix_keys16(seed0 + t, per)) for t in range(T)]
        return np.concatenate(bms + [np.zeros(16, np.uint8)]), kb_of([b.size for b in bms])

    true_arena, off = arena(0x5EED)
    decoy_arena, _ = arena(0xDEC0)
    k, f, m = oracle.synth_probe_queries(n, num_tables=T, keys_per_table=per)
    dk, df, _ = oracle.synth_probe_queries(n, seed=0xD00D, num_tables=T, keys_per_table=per)
    want = oracle.probe_multi(k, f, true_arena, off, bits_per_key=bpk)
    assert want[m.astype(bool)].all() and not want.all()
    wsb = L.adl_bloom_probe_batch_workspace_bytes(n, T, bpk, 16)
    assert wsb > 256, "the binned pipeline's workspace"

    def setup(case):
        bm = case.input(true_arena, decoy_arena)
        keys, fid = case.input(k, dk, pad=32), case.input(f, df)
        d_off = case.const(off)
        out, ws = case.output(n), case.workspace(wsb)

        def entry(s):
            ok(L.adl_bloom_probe_batch_device(keys.data_ptr(), None, n, 16, fid.data_ptr(), T, bm.data_ptr(),
                                              d_off.data_ptr(), None, bpk, out.data_ptr(), ws.data_ptr(), wsb,
                                              so.sptr(s)), "adl_bloom_probe_batch_device")

        return entry, lambda c: so.check(c.result(out, n), want, "answers")

    drive(setup)


# ---------------------------------------------------------------- hash and generators
@pytest.mark.parametrize("which", ["murmur3", "keys16", "varlen_lengths", "varlen_fill", "probe_queries"])
def test_hash_and_generators(dev, ab, oracle, which):
    L = ab.lib()
    n, seed = 4096, 0x5EED
    true, decoy = keys16(oracle, 31, n), keys16(oracle, 32, n)
    vdata, voffs = memo(("synth_varlen", n), lambda: oracle.synth_varlen(n, seed=seed))
    total = int(voffs[-1])

    def setup(case):
        if which == "murmur3":
            keys, out = case.input(true, decoy, pad=32), case.output(8 * n)
            call = lambda s: L.adl_bloom_murmur3_device(keys.data_ptr(), None, n, 16, ab.SEED1, ab.SEED2,
                                                        out.data_ptr(), so.sptr(s))
            want = [(out, oracle.murmur3_batch(true))]
        elif which == "keys16":
            out = case.output(16 * n)
            call = lambda s: L.adl_synth_keys16_device(out.data_ptr(), seed, 5, n, so.sptr(s))
            want = [(out, oracle.splitmix_keys16(seed, n, skip=5))]
        elif which == "varlen_lengths":
            out = case.output(4 * n)
            call = lambda s: L.adl_synth_varlen_lengths_device(out.data_ptr(), seed, n, 1.1, so.sptr(s))
            want = [(out, np.diff(voffs).astype(np.uint32))]
        elif which == "varlen_fill":
            out = case.output((total + 7) // 8 * 8)
            call = lambda s: L.adl_synth_varlen_fill_device(out.data_ptr(), seed, total, so.sptr(s))
            want = [(out, vdata[:total])]
        else:
            ko, fo, mo = case.output(16 * n), case.output(4 * n), case.output(n)
            call = lambda s: L.adl_synth_probe_queries_device(ko.data_ptr(), fo.data_ptr(), mo.data_ptr(), 0xFEED, 3,
                                                              n, 8, seed, 30_000, so.sptr(s))
            want = list(zip((ko, fo, mo), oracle.synth_probe_queries(n, q0=3, num_tables=8, keys_per_table=30_000)))

        def verify(c):
            for i, (o, w) in enumerate(want):
                so.check(c.result(o, w.nbytes), w, f"{which} output {i}")

        return (lambda s: ok(call(s), which)), verify

    drive(setup)


# ---------------------------------------------------------------- host-pointer entry points
@pytest.fixture(params=["delayed-stream", "stream-none"])
def hstream(request, dev):
    """hstream() -> the `stream` argument of the next host-pointer call: a
    non-blocking stream on which a delay has just been enqueued, or None (the
    thread's own stream)."""
    if request.param == "stream-none":
        yield lambda: None
        return
    s = dev.cuda.Stream()
    dev.cuda.synchronize()

    def delayed():
        so.delay(s)
        return s

    yield delayed
    s.synchronize()


def test_host_build(dev, ab, oracle, hstream):
    n = 20_011
    keys = keys16(oracle, 1, n)
    want = memo(("bm", 1, n, 10), lambda: oracle.keys2block(keys))
    so.check(ab.build_host(keys, stream=hstream()), want, "bitmap")


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("flags", [0, SKIP_DUP], ids=["segmented", "segmented_ex"])
def test_host_build_segmented(dev, ab, oracle, knobs, hstream, flags, pinned):
    """10 filters of 20 000 x 16 B keys with 1 MB pipeline groups: four groups,
    so the upload, build and download streams all run ahead of each other and
    both buffer parities are reused."""
    knobs.set("ADL_BLOOM_PIPE_MB", "1")
    sizes = [20_000] * 10
    kb = kb_of(sizes)
    keys = memo("seg-host-keys", lambda: with_repeats(keys16(oracle, 41, int(kb[-1]))))
    want = memo("seg-host-want", lambda: [oracle.keys2block(keys[int(kb[f]):int(kb[f + 1])]) for f in range(10)])
    boff = kb_of([w.size for w in want])  # packed back to back, as in a filter block
    total = int(boff[-1])
    if pinned:
        h_keys = dev.from_numpy(keys.copy()).pin_memory()
        out = dev.full((total,), 0xA5, dtype=dev.uint8).pin_memory()
    else:
        h_keys, out = keys, np.full(total, 0xA5, np.uint8)
    ab.build_segmented_host(h_keys, kb, out, boff[:-1], stream=hstream(), flags=flags)
    got = out.numpy() if pinned else out
    so.check(got, np.concatenate(want), "bitmaps")


def test_host_probe_and_filter_set(dev, ab, oracle, hstream):
    n, nq = 20_011, 5_000
    keys = keys16(oracle, 1, n)
    bm = memo(("bm", 1, n, 10), lambda: oracle.keys2block(keys))
    q = np.concatenate([keys[:nq // 2], keys16(oracle, 99, nq - nq // 2)])
    want = memo(("ans", 1, n, 10), lambda: oracle.probe(q, bm))
    so.check(ab.probe_host(q, bm, stream=hstream()), want, "adl_bloom_probe")
    fs = ab.FilterSet(bm, u64([0, bm.size]))
    try:
        so.check(fs.probe(q, stream=hstream()), want, "adl_bloom_filter_set_probe")
    finally:
        fs.close()


def test_host_verify(dev, ab, oracle, hstream):
    sizes = [1, 3000, 0, 7]
    kb = kb_of(sizes)
    keys = keys16(oracle, 51, int(kb[-1]))
    bms = [oracle.keys2block(keys[int(kb[f]):int(kb[f + 1])]) for f in range(len(sizes))]
    boff = kb_of([b.size for b in bms])
    arena = np.concatenate(bms)
    assert ab.verify(keys, kb, arena, boff, stream=hstream()) == (0, None)
    bad = arena.copy()
    bad[int(boff[1]):int(boff[2])] = 0  # filter 1 emptied: its 3000 keys are missing, key 1 first
    assert ab.verify(keys, kb, bad, boff, stream=hstream()) == (3000, 1)


def test_host_filter_cache(dev, ab, oracle, hstream):
    """filter_cache_build, then filter_cache_probe and _probe_fanout with 100
    queries (past what the resident server answers), all on `hstream`."""
    sizes = [1, 777, 3000]
    kb = kb_of(sizes)
    keys = keys16(oracle, 61, int(kb[-1]))
    bms = [oracle.keys2block(keys[int(kb[f]):int(kb[f + 1])]) for f in range(len(sizes))]
    cache = ab.FilterCache(4 << 20, max_tables=4)
    try:
        block, ticket = cache.build(keys, kb, stream=hstream())
        so.check(np.frombuffer(block, np.uint8),
                 np.frombuffer(oracle.filter_block_final([b.tobytes() for b in bms], 10), np.uint8), "filter block")
        cache.publish(ticket, b"t0")
        q = np.concatenate([keys[int(kb[2]):int(kb[2]) + 50], keys16(oracle, 62, 50)])
        want = oracle.probe(q, bms[2])
        assert want[:50].all() and not want.all()
        got, unc = cache.probe([b"t0"], np.zeros(100, np.uint32), q, filter=2, stream=hstream())
        assert unc == 0
        so.check(got, want, "adl_bloom_filter_cache_probe")
        # each key against t0 and against a table that is not cached (answers 1)
        got, unc = cache.probe_fanout([b"t0", b"nope"], np.arange(0, 201, 2), np.tile([0, 1], 100), q, filter=2,
                                      stream=hstream())
        assert unc == 100
        so.check(got, np.stack([want, np.ones(100, np.uint8)], 1).reshape(-1), "adl_bloom_filter_cache_probe_fanout")
    finally:
        cache.close()


# ---------------------------------------------------------------- two streams, two threads
A_SIZES = [300] * 256  # the claim layout in the default plan
B_N = 100_000          # the dense layout


def plan_lines(ab, capfd, counts):
    capfd.readouterr()
    assert ab.workspace_bytes(counts, 10) > 0
    return capfd.readouterr().err


def test_two_streams_one_thread(dev, ab, oracle, knobs, capfd):
    """Builder A (256 x 300 keys, claim layout, descriptors through the upload
    ring) on one stream and builder B (100 000 keys, dense layout) on another,
    interleaved three times with fresh keys and no synchronise: whatever the
    calling thread keeps between builds must not tie one build to the other's
    stream or layout."""
    knobs.set("ADL_BLOOM_DEBUG", "1")
    assert "(claim)" in plan_lines(ab, capfd, A_SIZES) and "(claim)" not in plan_lines(ab, capfd, [B_N])
    knobs.unset("ADL_BLOOM_DEBUG")
    kb = kb_of(A_SIZES)
    na = int(kb[-1])
    a, b = ab.SegmentedBuilder(kb), ab.Builder(B_N)
    ka = [dev.from_numpy(keys16(oracle, 70 + r, na)).cuda() for r in range(3)]
    kbk = [dev.from_numpy(keys16(oracle, 80 + r, B_N)).cuda() for r in range(3)]
    cur_a, cur_b = dev.from_numpy(keys16(oracle, 7, na)).cuda(), dev.from_numpy(keys16(oracle, 8, B_N)).cuda()
    ha = [dev.full((a.out.numel(),), 0xA5, dtype=dev.uint8).pin_memory() for _ in range(3)]
    hb = [dev.full((b.nbytes,), 0xA5, dtype=dev.uint8).pin_memory() for _ in range(3)]
    for t in (a.out, b.bitmap):
        t.fill_(0xA5)
    for t in (a.ws, b.ws):
        t.fill_(0x5A)
    s1, s2 = dev.cuda.Stream(), dev.cuda.Stream()
    dev.cuda.synchronize()
    so.delay(s1)
    so.delay(s2)
    for r in range(3):
        with dev.cuda.stream(s1):
            cur_a.copy_(ka[r])
        a.build(cur_a, stream=s1)
        with dev.cuda.stream(s1):
            ha[r].copy_(a.out, non_blocking=True)
        with dev.cuda.stream(s2):
            cur_b.copy_(kbk[r])
        b.build(cur_b, stream=s2)
        with dev.cuda.stream(s2):
            hb[r].copy_(b.bitmap[:b.nbytes], non_blocking=True)
    s1.synchronize()
    s2.synchronize()
    for r in range(3):
        so.check(hb[r].numpy(), oracle.keys2block(keys16(oracle, 80 + r, B_N)), f"B round {r}")
        # all 256 bitmaps of A at their offsets, the 16-byte pad after each written as zero
        hk, want = keys16(oracle, 70 + r, na), np.zeros(a.out.numel(), np.uint8)
        for f in range(len(A_SIZES)):
            o = int(a.boff[f])
            want[o:o + int(a.sizes[f])] = oracle.keys2block(hk[int(kb[f]):int(kb[f + 1])])
        so.check(ha[r].numpy(), want, f"A round {r}")


def test_two_threads(dev, ab, oracle):
    """Two Python threads (ctypes releases the GIL), each with its own stream
    and buffers: 10 iterations of a segmented build followed on the same stream
    by probe_multi over what it built.  probe_multi takes contiguous ranges, so
    the 16-byte-aligned bitmaps are listed as filters 0, 2, 4, ... and the pad
    bytes between them as the odd filters, which no query names."""
    L = ab.lib()
    sizes, bpk, nq, iters = [500, 1, 1200, 37, 64, 800], 10, 2_000, 10
    F = len(sizes)
    kb = kb_of(sizes)
    n = int(kb[-1])
    exact = [ab.bitmap_bytes(c, bpk) for c in sizes]
    boff = kb_of([ab.bitmap_alloc_bytes(c, bpk) for c in sizes])
    ranges = np.zeros(2 * F + 1, np.uint64)
    ranges[0:2 * F:2], ranges[1:2 * F:2], ranges[2 * F] = boff[:-1], boff[:-1] + u64(exact), boff[-1]
    wsb = ab.workspace_bytes(sizes, bpk)
    errors = []
    kb_i, sizes_i = kb.astype(np.int64), np.array(sizes, np.int64)

    def plan(t, i):
        keys = keys16(oracle, 1000 * (t + 1) + i, n)
        rng = np.random.default_rng(t * 100 + i)
        q = keys16(oracle, 5000 * (t + 1) + i, nq).copy()
        fid = rng.integers(0, F, nq).astype(np.uint32)
        ins = np.nonzero(rng.integers(0, 2, nq))[0]
        q[ins] = keys[kb_i[fid[ins]] + rng.integers(0, 1 << 30, ins.size) % sizes_i[fid[ins]]]
        want = np.zeros(nq, np.uint8)
        for f in range(F):
            sel = fid == f
            assert sel.any()
            want[sel] = oracle.probe(q[sel], oracle.keys2block(keys[int(kb[f]):int(kb[f + 1])]))
        return keys, q, fid * 2, want

    plans = [[plan(t, i) for i in range(iters)] for t in range(2)]

    def worker(t):
        try:
            dev.cuda.set_device(0)
            s = dev.cuda.Stream()
            d_keys = dev.empty(16 * n + 32, dtype=dev.uint8, device="cuda")
            d_q = dev.empty(16 * nq + 32, dtype=dev.uint8, device="cuda")
            d_fid = dev.empty(4 * nq, dtype=dev.uint8, device="cuda")
            d_rng = dev.from_numpy(ranges.view(np.int64)).cuda()
            out = dev.full((int(boff[-1]),), 0xA5, dtype=dev.uint8, device="cuda")
            ws = dev.full((wsb,), 0x5A, dtype=dev.uint8, device="cuda")
            ans = dev.full((nq,), 0xA5, dtype=dev.uint8, device="cuda")
            h_ans = dev.full((nq,), 0xA5, dtype=dev.uint8).pin_memory()
            for i, (keys, q, fid2, want) in enumerate(plans[t]):
                hk, hq, hf = (dev.from_numpy(x.reshape(-1).view(np.uint8)).pin_memory() for x in (keys, q, fid2))
                with dev.cuda.stream(s):
                    d_keys[:16 * n].copy_(hk, non_blocking=True)
                    d_q[:16 * nq].copy_(hq, non_blocking=True)
                    d_fid.copy_(hf, non_blocking=True)
                ok(L.adl_bloom_build_segmented_device_ex(d_keys.data_ptr(), None, 16, kb.ctypes.data, F, bpk,
                                                         out.data_ptr(), boff.ctypes.data, 0, ws.data_ptr(), wsb,
                                                         so.sptr(s)), "build")
                ok(L.adl_bloom_probe_multi_device(d_q.data_ptr(), None, nq, 16, d_fid.data_ptr(), 2 * F,
                                                  out.data_ptr(), d_rng.data_ptr(), bpk, ans.data_ptr(), so.sptr(s)),
                   "probe_multi")
                with dev.cuda.stream(s):
                    h_ans.copy_(ans, non_blocking=True)
                s.synchronize()
                so.check(h_ans.numpy(), want, f"thread {t} iteration {i}")
        except BaseException as e:  # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    dev.cuda.synchronize()
    assert not errors, errors


# ---------------------------------------------------------------- adl_bloom_build_positions
@pytest.mark.parametrize("order", ["A-then-B", "B-then-A"])
def test_build_positions_uses_the_workspaces_own_layout(dev, ab, oracle, knobs, capfd, order):
    """Two builders on one thread, one in the claim layout and one in the dense
    layout: positions() of either, asked after the other has built, decodes its
    own workspace's table.  With the repeated-pair table off every key writes
    k = 6 positions."""
    knobs.set("ADL_BLOOM_HASH_DEDUP", "0")
    knobs.set("ADL_BLOOM_DEBUG", "1")
    assert "(claim)" in plan_lines(ab, capfd, A_SIZES) and "(claim)" not in plan_lines(ab, capfd, [B_N])
    knobs.unset("ADL_BLOOM_DEBUG")
    kb = kb_of(A_SIZES)
    a, b = ab.SegmentedBuilder(kb), ab.Builder(B_N)
    ka = dev.from_numpy(keys16(oracle, 70, int(kb[-1]))).cuda()
    kbk = dev.from_numpy(keys16(oracle, 80, B_N)).cuda()
    first, second = ((a, ka), (b, kbk)) if order == "A-then-B" else ((b, kbk), (a, ka))
    first[0].build(first[1])
    second[0].build(second[1])
    want = {id(a): 6 * int(kb[-1]), id(b): 6 * B_N}
    got_first, got_second = first[0].positions(), second[0].positions()
    print(f"positions: {order}: first built {got_first} (want {want[id(first[0])]}), "
          f"second built {got_second} (want {want[id(second[0])]})")
    assert got_first == want[id(first[0])]
    assert got_second == want[id(second[0])]
    so.check(b.bitmap[:b.nbytes].cpu().numpy(), oracle.keys2block(keys16(oracle, 80, B_N)), "B's bitmap")


@pytest.mark.parametrize("where", ["null-stream", "stream"])
def test_build_positions_is_ordered_after_the_build(dev, ab, oracle, knobs, where):
    """build(stream=X) behind the delay on X, then positions(stream=X) with no
    synchronise in between: the readback runs on the stream the build ran on
    (stream None: torch's default stream, handle 0, the null stream), so it sees
    the build's table, not the 0x5A bytes the workspace held before."""
    knobs.set("ADL_BLOOM_HASH_DEDUP", "0")
    b = ab.Builder(B_N)
    keys = dev.from_numpy(keys16(oracle, 80, B_N)).cuda()
    b.ws.fill_(0x5A)
    b.bitmap.fill_(0xA5)
    s = dev.cuda.Stream() if where == "stream" else None
    dev.cuda.synchronize()
    if s is None:
        assert dev.cuda.current_stream().cuda_stream == 0
    so.delay(s if s is not None else dev.cuda.current_stream())
    b.build(keys, stream=s)
    try:
        got = b.positions(stream=s)
    except ab.AdlBloomError as e:  # the workspace did not hold a build's table yet
        got = f"status {e.status}"
    print(f"positions after build on the {where}: {got} (want {6 * B_N})")
    assert got == 6 * B_N
    dev.cuda.synchronize()
    so.check(b.bitmap[:b.nbytes].cpu().numpy(), oracle.keys2block(keys16(oracle, 80, B_N)), "bitmap")


# ---------------------------------------------------------------- the adlbloom wrappers on a stream that is not current
def delayed_stream(dev):
    """A fresh non-blocking stream with the delay on it, and an event right after the delay."""
    s = dev.cuda.Stream()
    dev.cuda.synchronize()
    so.delay(s)
    ev = dev.cuda.Event()
    ev.record(s)
    return s, ev


@pytest.mark.parametrize("which", ["build", "probe", "probe_batch"])
def test_wrapper_allocates_for_the_stream_it_was_given(dev, ab, oracle, monkeypatch, which):
    """build / probe / probe_batch with stream = a delayed stream that is not
    current: the result is right once that stream has run, the call did not
    wait, and the device buffers the wrapper took and dropped on return (the
    workspaces) are not handed to an allocation on the current stream while
    the call's work is still pending -- they belong to the given stream's pool."""
    n, bpk, nq = 20_011, 10, 5_000
    true, decoy = keys16(oracle, 1, n), keys16(oracle, 2, n)
    bm_want = memo(("bm", 1, n, bpk), lambda: oracle.keys2block(true, bits_per_key=bpk))
    q = np.concatenate([true[:nq // 2], keys16(oracle, 99, nq - nq // 2)])
    ans = memo(("ans", 1, n, bpk), lambda: oracle.probe(q, bm_want, bits_per_key=bpk))
    src = dev.from_numpy(true if which == "build" else q).cuda()
    cur = dev.from_numpy(decoy if which == "build" else np.ascontiguousarray(q[::-1])).cuda()
    d_bm = dev.from_numpy(np.concatenate([bm_want, np.zeros(16, np.uint8)])).cuda()
    d_off = dev.from_numpy(np.array([0, bm_want.size], np.int64)).cuda()
    d_fid = dev.zeros(nq, dtype=dev.int32, device="cuda")
    want = bm_want if which == "build" else ans
    host = dev.full((want.size,), 0xA5, dtype=dev.uint8).pin_memory()

    def call(stream):
        if which == "build":
            return ab.build(cur, bits_per_key=bpk, stream=stream)
        if which == "probe":
            return ab.probe(cur, d_bm, nbytes=bm_want.size, bits_per_key=bpk, stream=stream)
        return ab.probe_batch(cur, d_fid, d_bm, d_off, bits_per_key=bpk, stream=stream)

    call(None)  # warm-up on the current stream
    taken, orig = [], ab.empty_device

    def recording(nbytes, device="cuda"):
        t = orig(nbytes, device)
        taken.append((t.data_ptr(), t.numel()))
        return t

    monkeypatch.setattr(ab, "empty_device", recording)
    s, after_delay = delayed_stream(dev)
    with dev.cuda.stream(s):
        cur.copy_(src)
    res = call(s)
    dropped = [(p, sz) for p, sz in taken if p != res.data_ptr()]
    assert dropped or which == "probe"  # (probe has no workspace)
    again = [dev.empty(sz, dtype=dev.uint8, device="cuda") for _, sz in dropped]
    assert not {t.data_ptr() for t in again} & {p for p, _ in dropped}
    assert not after_delay.query(), "the wrapper waited for the stream"
    with dev.cuda.stream(s):
        host.copy_(res, non_blocking=True)
    s.synchronize()
    so.check(host.numpy(), want, which)


@pytest.mark.parametrize("which", ["build_segmented", "build_filter_block"])
def test_wrapper_synchronises_the_stream_it_was_given(dev, ab, oracle, which):
    """build_segmented and build_filter_block end the lifetime of their
    workspace with the call, so they wait -- for the stream they were given,
    not for the current one: at return the delay on that stream is over and the
    result, read on the current stream, is the oracle's."""
    sizes = [0, 1, 300, 7, 2000]
    kb = kb_of(sizes)
    n = int(kb[-1])
    true, decoy = keys16(oracle, 91, n), keys16(oracle, 92, n)
    bms = [oracle.keys2block(true[int(kb[f]):int(kb[f + 1])]) for f in range(len(sizes))]
    src, cur = dev.from_numpy(true).cuda(), dev.from_numpy(decoy).cuda()
    s, after_delay = delayed_stream(dev)
    with dev.cuda.stream(s):
        cur.copy_(src)
    if which == "build_segmented":
        out, boff, nbytes = ab.build_segmented(cur, kb, stream=s)
        assert after_delay.query(), "returned with the given stream's work still pending"
        want = np.zeros(out.numel(), np.uint8)
        for f, b in enumerate(bms):
            want[int(boff[f]):int(boff[f]) + b.size] = b
        so.check(out.cpu().numpy(), want, "bitmaps")
    else:
        block = ab.build_filter_block(cur, kb, stream=s)
        assert after_delay.query(), "returned with the given stream's work still pending"
        so.check(block.cpu().numpy(),
                 np.frombuffer(oracle.filter_block_final([b.tobytes() for b in bms], 10), np.uint8), "filter block")


def test_synth_varlen_wrapper_runs_its_prefix_sum_on_the_given_stream(dev, ab, oracle):
    """synth_varlen is two launches with a torch prefix sum of the lengths in
    between: all three on the given stream, behind its delay."""
    n, seed = 4096, 0x5EED
    want_d, want_o = memo(("synth_varlen", n), lambda: oracle.synth_varlen(n, seed=seed))
    total = int(want_o[-1])
    s, _ = delayed_stream(dev)
    data, offs = ab.synth_varlen(n, seed=seed, stream=s)
    with dev.cuda.stream(s):
        h_o, h_d = offs.cpu(), data.cpu()
    so.check(h_o.numpy().view(np.uint64), want_o, "offsets")
    so.check(h_d.numpy()[:total], want_d[:total], "key bytes")
