"""GPU: the large-batch probe with a probe count per filter
(adl_bloom_probe_batch_k_device, csrc/probe_binned.hip).

One arena holds filters the oracle built under bits_per_key 1, 3, 10, 11 and 44
(k = 1, 2, 6, 7 and 30): filters of under 2^20 bits (one tile: pb_bin's T == 1
branch) at k = 2, 6 and 30; filters of exactly two tiles at k = 2, 6 (13 200
keys at bpk 10) and 30 (3 000 keys at bpk 44); 110 000 keys at bpk 10, 100 000 at
bpk 11 and 30 000 at bpk 44, which are 9 to 11 tiles each (the reference's
bitmap is n * bpk + 7 bytes, src/filter_block.cpp:9-33, not bits); a range of 0
bytes and the 7-byte bitmap of no keys.  Ids come from [0, F + 2) and half the
queries bound for a filter are members of it.  The plan is made from max_k = 30 (chunks of 1280 queries), so
every populated filter spans several chunks, each writing k_f entries a query
into a region sized for 30.

Every answer equals BloomFilter::IsKeyExists (src/filter_block.cpp:49-62) with
the filter's own bits_per_key -- one oracle.probe_multi per distinct
bits_per_key (tests/mixedk.py) -- with `==`, and the same call forced onto the
direct kernel with ADL_BLOOM_PROBE_BATCH_MAX_K=1.  The `adl_bloom
probe_batch_k:` line (ADL_BLOOM_DEBUG=1) says which path ran.

n = 2^20 + 777: the smallest batch the pipeline takes, with a ragged last block
of 8192 and, for keys that are not 16-byte keys, a ragged last run of 512.
"""
import gc
import re

import numpy as np
import pytest

import probekeys as pk
import streamorder as so
from guardband import Guarded, check_all
from mixedk import MixedBatch, MixedFilters

pytestmark = pytest.mark.gpu

N = (1 << 20) + 777
VAR_MIN = "ADL_BLOOM_PROBE_BATCH_VAR_MIN"
MAX_K = "ADL_BLOOM_PROBE_BATCH_MAX_K"
LINE = re.compile(r"adl_bloom probe_batch_k: (binned|direct) \(([^)]*)\), kmax=(\d+), launches=(\d+)")
ADL_ERR_WORKSPACE = -5
# (members, bits_per_key); None: a range of 0 bytes; 0: the 7-byte bitmap of no keys
SPEC = [(300, 1), (40_000, 1), (5_000, 3), (60_000, 3), (5_000, 10), (110_000, 10), (3_000, 11), (100_000, 11),
        (2_000, 44), (30_000, 44), (None, 10), (0, 10), (13, 44), (1, 3), (13_200, 10), (3_000, 44)]
SPEC_K7 = [s for s in SPEC if s[1] != 44]  # the largest k present is 7


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


@pytest.fixture(autouse=True)
def release(dev):
    yield
    gc.collect()
    dev.cuda.synchronize()
    dev.cuda.empty_cache()


@pytest.fixture(scope="module")
def base(oracle):
    """16-byte keys over the filters of SPEC."""
    flt = MixedFilters(oracle, SPEC, seed=0xA11)
    assert sorted(set(flt.k.tolist())) == [1, 2, 6, 7, 30]
    bits = [b.size * 8 for b in flt.bms]
    for t, k in ((2, 2), (4, 6), (8, 30)):
        assert flt.k[t] == k and 0 < bits[t] < 1 << 20
    for t, k in ((3, 2), (14, 6), (15, 30)):  # two tiles
        assert flt.k[t] == k and 1 << 20 < bits[t] <= 2 << 20
    for t, k in ((5, 6), (7, 7), (9, 30)):  # several
        assert flt.k[t] == k and 8 << 20 < bits[t] < 12 << 20
    assert bits[10] == 0 and bits[11] == 56
    return MixedBatch(oracle, flt, N, seed=21)


def _d(dev, a):
    """Host array -> device tensor (uint64 / uint32 travel as int64 / int32)."""
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return dev.from_numpy(a).cuda()


def same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} answers differ, the first at {bad[0]}"
    assert np.array_equal(got, want)


def lines(capfd):
    return [(path, shape, int(kmax)) for path, shape, kmax, _ in LINE.findall(capfd.readouterr().err)]


def inputs(dev, b, arena=None, begin=None, end=None):
    """The device arguments of ab.probe_batch_k for batch b."""
    flt = b.flt
    if b.stride is None:
        keys, kw = _d(dev, b.data), {"offsets": _d(dev, b.off)}
    else:
        keys, kw = _d(dev, b.keys), {}
    if end is not None:
        kw["bitmap_end"] = _d(dev, end)
    return (keys, _d(dev, b.fid), _d(dev, flt.arena if arena is None else arena),
            _d(dev, flt.off if begin is None else begin), _d(dev, flt.k)), kw


def both_paths(dev, ab, knobs, capfd, b, shape, max_k=30, **kw):
    """The call on the binned pipeline and forced direct, each against the oracle and each other."""
    args, kws = inputs(dev, b, **kw)
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(MAX_K, 30)
    capfd.readouterr()
    got = ab.probe_batch_k(*args, max_k, **kws).cpu().numpy()
    assert lines(capfd) == [("binned", shape, max_k)]
    knobs.set(MAX_K, 1)
    direct = ab.probe_batch_k(*args, max_k, **kws).cpu().numpy()
    direct_shape = "stride 16" if shape == "keys16" else shape
    assert lines(capfd) == [("direct", direct_shape, max_k)]
    knobs.set(MAX_K, 30)
    same(direct, b.want, "direct kernel")
    same(got, b.want, "binned pipeline")
    assert got.tobytes() == direct.tobytes()
    return got


# ---------------------------------------------------------------- 1 the three key shapes
def test_keys16(dev, ab, knobs, capfd, base):
    both_paths(dev, ab, knobs, capfd, base, "keys16")


def test_ranges_in_shuffled_arena_order(dev, ab, knobs, capfd, base):
    arena, begin, end = base.flt.scattered()
    assert not np.array_equal(np.argsort(begin), np.arange(base.flt.F))
    both_paths(dev, ab, knobs, capfd, base, "keys16", arena=arena, begin=begin, end=end)


def test_varlen_keys(dev, ab, oracle, knobs, capfd):
    """Zipf 8-256 B keys (tests/probekeys.py) with the knob forced."""
    knobs.set(VAR_MIN, 1)
    flt = MixedFilters(oracle, SPEC, seed=0xA12, stride=None)
    b = MixedBatch(oracle, flt, N, seed=22, stride=None, lens=pk.zipf_lengths(oracle, N, 22))
    both_paths(dev, ab, knobs, capfd, b, "var")


def test_stride_24(dev, ab, oracle, knobs, capfd):
    knobs.set(VAR_MIN, 1)
    flt = MixedFilters(oracle, SPEC, seed=0xA13, stride=24)
    b = MixedBatch(oracle, flt, N, seed=23, stride=24)
    both_paths(dev, ab, knobs, capfd, b, "stride 24")


# ---------------------------------------------------------------- 2 against the uniform entry point
def test_all_6_equals_the_uniform_call(dev, ab, oracle, knobs, capfd):
    """d_filter_k all 6: the bytes of adl_bloom_probe_batch_device(bits_per_key = 10) on the
    same inputs, with max_k = 6 (the uniform plan) and with max_k = 30 (a smaller C)."""
    flt = pk.Filters(oracle, [5000, 13, None, 110_000, 1, 0, 300], bpk=10, seed=0xA14, stride=16)
    data, lens, fid, member = pk.queries(flt, N, np.full(N, 16), 24)
    keys = data[:N * 16].reshape(N, 16)
    want = oracle.probe_multi(keys, fid, flt.arena, flt.off, bits_per_key=10)
    assert want[member].all() and not want.all()
    d_keys, d_fid, d_arena, d_off = _d(dev, keys), _d(dev, fid), _d(dev, flt.arena), _d(dev, flt.off)
    d_k = dev.full((flt.F,), 6, dtype=dev.uint8, device="cuda")
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(MAX_K, 30)
    uniform = ab.probe_batch(d_keys, d_fid, d_arena, d_off, bits_per_key=10).cpu().numpy()
    same(uniform, want, "probe_batch")
    for max_k in (6, 30):
        capfd.readouterr()
        got = ab.probe_batch_k(d_keys, d_fid, d_arena, d_off, d_k, max_k).cpu().numpy()
        assert lines(capfd) == [("binned", "keys16", max_k)]
        same(got, want, f"max_k {max_k}")
        assert got.tobytes() == uniform.tobytes()


@pytest.mark.parametrize("max_k", [7, 12])
def test_max_k_exact_and_larger(dev, ab, oracle, knobs, capfd, max_k):
    """max_k exactly the largest k present (7), and larger than it."""
    flt = MixedFilters(oracle, SPEC_K7, seed=0xA15)
    assert int(flt.k.max()) == 7
    b = MixedBatch(oracle, flt, N, seed=25)
    both_paths(dev, ab, knobs, capfd, b, "keys16", max_k=max_k)


# ---------------------------------------------------------------- 3 buffer contracts
def _call(ab, b, d, max_k, out_ptr, ws_ptr, wsb, stream=None):
    keys, fid, arena, off, k = d
    return ab.lib().adl_bloom_probe_batch_k_device(keys.data_ptr(), None, b.n, 16, fid.data_ptr(), b.flt.F,
                                                   arena.data_ptr(), off.data_ptr(), None, k.data_ptr(), max_k, out_ptr,
                                                   ws_ptr, wsb, ab._stream() if stream is None else stream)


def test_exact_workspace_in_guard_bands(dev, ab, knobs, base):
    """The workspace at exactly the promised size, 256-byte aligned; d_out at an odd
    address; all inside 0xA5 guard bands."""
    knobs.set(MAX_K, 30)
    d, _ = inputs(dev, base)
    wsb = ab.lib().adl_bloom_probe_batch_k_workspace_bytes(N, base.flt.F, 30, 16)
    assert wsb > 256
    ws = Guarded(wsb, 256, name="d_workspace")
    out = Guarded(N, 8, skew=3, name="d_out")
    assert ws.ptr % 256 == 0 and out.ptr % 2 == 1
    rc = _call(ab, base, d, 30, out.ptr, ws.ptr, wsb)
    assert rc == 0, rc
    dev.cuda.synchronize()
    same(out.numpy(), base.want, "answers")
    check_all(out, ws)
    assert not bool((ws.view == ws.fill).all())  # the binned pipeline ran


def test_workspace_one_byte_short(dev, ab, knobs, base):
    knobs.set(MAX_K, 30)
    d, _ = inputs(dev, base)
    wsb = ab.lib().adl_bloom_probe_batch_k_workspace_bytes(N, base.flt.F, 30, 16)
    ws = Guarded(wsb - 1, 256, name="d_workspace")
    out = Guarded(N, 8, skew=3, name="d_out")
    rc = _call(ab, base, d, 30, out.ptr, ws.ptr, wsb - 1)
    assert rc == ADL_ERR_WORKSPACE, rc
    dev.cuda.synchronize()
    check_all(out, ws)
    assert bool((out.view == out.fill).all()) and bool((ws.view == ws.fill).all())


# ---------------------------------------------------------------- 4 stream order
def test_stream_order(dev, ab, knobs, base):
    """On a fresh non-blocking stream behind the delay (tests/streamorder.py): the
    call returns while the delay runs and the answers are exact."""
    knobs.set(MAX_K, 30)
    L, flt = ab.lib(), base.flt
    rng = np.random.default_rng(9)
    decoy = rng.integers(0, 256, base.total, dtype=np.uint8)  # no members
    decoy_fid = ((base.fid + 1) % (flt.F + 2)).astype(np.uint32)
    wsb = L.adl_bloom_probe_batch_k_workspace_bytes(N, flt.F, 30, 16)
    assert wsb > 256, "the binned pipeline's workspace"

    def setup(case):
        keys, fid = case.input(base.data[:base.total], decoy, pad=32), case.input(base.fid, decoy_fid)
        bm, boff, dk = case.const(flt.arena), case.const(flt.off), case.const(flt.k)
        out, ws = case.output(N), case.workspace(wsb)

        def entry(s):
            rc = L.adl_bloom_probe_batch_k_device(keys.data_ptr(), None, N, 16, fid.data_ptr(), flt.F, bm.data_ptr(),
                                                  boff.data_ptr(), None, dk.data_ptr(), 30, out.data_ptr(),
                                                  ws.data_ptr(), wsb, so.sptr(s))
            assert rc == 0, rc

        return entry, lambda c: so.check(c.result(out, N), base.want, "answers")

    warm = so.Case()
    entry, _ = setup(warm)
    entry(None)
    dev.cuda.synchronize()
    case = so.Case()
    entry, verify = setup(case)
    case.run(entry)
    assert case.returned_early, "the entry point came back only after the delay: it waits for the stream"
    verify(case)


# ---------------------------------------------------------------- 5 determinism
def test_same_bytes_twice_into_dirty_buffers(dev, ab, knobs, base):
    knobs.set(MAX_K, 30)
    args, kw = inputs(dev, base)
    wsb = ab.lib().adl_bloom_probe_batch_k_workspace_bytes(N, base.flt.F, 30, 16)
    outs = []
    for fill in (0xA5, 0x3C):
        out = dev.full((N + 64,), fill, dtype=dev.uint8, device="cuda")
        ws = dev.full((wsb,), fill, dtype=dev.uint8, device="cuda")
        ab.probe_batch_k(*args, 30, out=out, workspace=ws, **kw)
        got = out.cpu().numpy()
        assert (got[N:] == fill).all()
        outs.append(got[:N].tobytes())
    assert outs[0] == outs[1]
    assert np.array_equal(np.frombuffer(outs[0], np.uint8), base.want)
