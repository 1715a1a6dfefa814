"""GPU: the large-batch probe (adl_bloom_probe_batch_device) over keys that are
not aligned 16-byte keys.

Variable-length keys (d_offsets) and fixed strides other than 16 take the
tile-binned pipeline from ADL_BLOOM_PROBE_BATCH_VAR_MIN queries on:
hash_run_pairs_kernel (csrc/hash_pairs.hip) hashes runs of 512 queries from LDS,
sorted by length, and leaves each (h1, h2) at its query's index; the rest of
the pipeline is the 16-byte one.  Every answer here equals
BloomFilter::IsKeyExists (src/filter_block.cpp:49-62) per query --
oracle.probe_multi -- with `==`, and the direct kernel's on the same device
inputs.  The knob forces each path; the `adl_bloom probe_batch:` line
(ADL_BLOOM_DEBUG=1) says which one ran.

n = 2^20 + 777 unless a case says otherwise: the smallest batch the pipeline
takes, with a ragged last run of 512 and a ragged last block of 8192.
Filters are built by the oracle from variable-length member keys
(tests/probekeys.py); half the queries are members of their filter, ids come
from [0, F + 2), one filter has no bytes and one no keys.
"""
import gc
import re

import numpy as np
import pytest

import probekeys as pk
import streamorder as so
from guardband import Guarded, Poisoned, check_all

pytestmark = pytest.mark.gpu

N = (1 << 20) + 777
KNOB = "ADL_BLOOM_PROBE_BATCH_VAR_MIN"
LINE = re.compile(r"adl_bloom probe_batch: (binned|direct) \(([^)]*)\)")
ADL_ERR_WORKSPACE = -5
SIZES = [5000, 13, None, 40_000, 1, 0, 300]  # None: a filter of 0 bytes; 0: the 7-byte bitmap of no keys
BIG_BYTES = (1 << 32) + (1 << 26)


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


class Batch:
    """A query batch over `flt` and the oracle's answers (computed once, read-only)."""

    def __init__(self, oracle, flt, data, lens, fid, member=None, stride=None):
        self.flt, self.data, self.lens, self.fid, self.member, self.stride = flt, data, lens, fid, member, stride
        self.n = len(fid)
        self.off = pk.offsets_of(lens)
        self.total = int(self.off[-1])
        if stride is None:
            self.want = oracle.probe_multi(data, fid, flt.arena, flt.off, offsets=self.off, bits_per_key=flt.bpk)
        else:
            self.keys = data[:self.total].reshape(self.n, stride)
            self.want = oracle.probe_multi(self.keys, fid, flt.arena, flt.off, bits_per_key=flt.bpk)
        if member is not None:
            has_members = np.concatenate([flt.counts, [0, 0]])[fid] > 0
            assert self.want[member].all() and member.sum() > 0.45 * has_members.sum() and not self.want.all()
        assert not self.want[fid >= flt.F].any()
        for a in (self.data, self.fid, self.off, self.want):
            a.flags.writeable = False


def var_batch(oracle, n=N, bpk=10, seed=7, lens=None, fixed=None, sizes=SIZES):
    flt = pk.Filters(oracle, sizes, bpk=bpk, seed=0x5EED + bpk)
    lens = pk.zipf_lengths(oracle, n, seed) if lens is None else lens
    data, lens, fid, member = pk.queries(flt, n, lens, seed, fixed=fixed)
    return Batch(oracle, flt, data, lens, fid, member)


def stride_batch(oracle, stride, n=N, bpk=10):
    sizes = SIZES if stride > 1 else [20, 3, None, 40, 1, 0, 30]
    flt = pk.Filters(oracle, sizes, bpk=bpk, seed=0xABC + stride, stride=stride)
    data, lens, fid, member = pk.queries(flt, n, np.full(n, stride), 100 + stride)
    return Batch(oracle, flt, data, lens, fid, member, stride=stride)


@pytest.fixture(scope="module")
def base(oracle):
    """The Zipf 8-256 B batch most cases use."""
    return var_batch(oracle)


def _d(dev, a):
    """Host array -> device tensor (uint64 / uint32 travel as int64 / int32)."""
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)  # (a shared, read-only input: a copy)
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
    return LINE.findall(capfd.readouterr().err)


def at_offset(dev, host_bytes, align):
    """A device copy of host_bytes whose first byte is at an address = align (mod 256)."""
    buf = dev.empty(256 + host_bytes.size + 64, dtype=dev.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[align:align + host_bytes.size]
    view.copy_(dev.from_numpy(np.ascontiguousarray(host_bytes)))
    return view


def run_var(dev, ab, b, n=None, data=None, off=None):
    """probe_batch and the direct kernel on the same device inputs against the oracle's answers."""
    n = b.n if n is None else n
    d_data = _d(dev, b.data) if data is None else data
    d_off = _d(dev, b.off[:n + 1]) if off is None else off
    d_fid, d_arena, d_boff = _d(dev, b.fid[:n]), _d(dev, b.flt.arena), _d(dev, b.flt.off)
    got = ab.probe_batch(d_data, d_fid, d_arena, d_boff, offsets=d_off, bits_per_key=b.flt.bpk).cpu().numpy()
    direct = ab.probe_multi(d_data, d_fid, d_arena, d_boff, offsets=d_off, bits_per_key=b.flt.bpk).cpu().numpy()
    same(direct, b.want[:n], "direct kernel")
    same(got, b.want[:n], "probe_batch")
    return got


def run_stride(dev, ab, b, n=None, align=0):
    n = b.n if n is None else n
    d_keys = at_offset(dev, b.keys[:n].reshape(-1), align).view(n, b.stride)
    assert d_keys.data_ptr() % 16 == align % 16
    d_fid, d_arena, d_boff = _d(dev, b.fid[:n]), _d(dev, b.flt.arena), _d(dev, b.flt.off)
    got = ab.probe_batch(d_keys, d_fid, d_arena, d_boff, bits_per_key=b.flt.bpk).cpu().numpy()
    direct = ab.probe_multi(d_keys, d_fid, d_arena, d_boff, bits_per_key=b.flt.bpk).cpu().numpy()
    same(direct, b.want[:n], "direct kernel")
    same(got, b.want[:n], "probe_batch")
    return got


# ---------------------------------------------------------------- 1 path
def test_path(dev, ab, oracle, knobs, capfd, base):
    """Which path a batch takes: binned for var-len keys and a 24-byte stride
    with the knob at 1; direct with the knob at 0, one query under 2^20, and
    for 16-byte keys at an unaligned pointer.  Exact answers every time."""
    b24, b16 = stride_batch(oracle, 24), stride_batch(oracle, 16)
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    run_var(dev, ab, base)
    assert lines(capfd) == [("binned", "var")]
    run_stride(dev, ab, b24)
    assert lines(capfd) == [("binned", "stride 24")]
    run_var(dev, ab, base, n=(1 << 20) - 1)
    assert lines(capfd) == [("direct", "var")]
    run_stride(dev, ab, b24, n=(1 << 20) - 1)
    assert lines(capfd) == [("direct", "stride 24")]
    run_stride(dev, ab, b16, align=1)
    assert lines(capfd) == [("direct", "stride 16")]
    run_stride(dev, ab, b16, align=0)
    assert lines(capfd) == [("binned", "keys16")]
    knobs.set(KNOB, 0)
    capfd.readouterr()
    run_var(dev, ab, base)
    assert lines(capfd) == [("direct", "var")]
    run_stride(dev, ab, b24)
    assert lines(capfd) == [("direct", "stride 24")]


# ---------------------------------------------------------------- 2 lengths and bytes
SPECIAL = list(range(71)) + [255, 256, 300, 510, 511, 512, 1000]  # every len % 4 tail; the 511 bin clamp


@pytest.mark.parametrize("bpk", [10, 3])
def test_lengths_and_bytes(dev, ab, oracle, knobs, capfd, bpk):
    """k = 6 (pb_bin_kernel<6>) and k = 2 (<0>): every length 0..70 and the
    lengths around the bin clamp, side by side in one run and one to a run;
    two whole runs of empty keys; an empty key between keys that lie past the
    staging, and one between staged keys; the rest Zipf 8-256 B."""
    lens = pk.zipf_lengths(oracle, N, 11)
    fixed = np.zeros(N, bool)

    def put(at, values):
        lens[at:at + len(values)] = values
        fixed[at:at + len(values)] = True

    put(3 * pk.RUN + 5, SPECIAL)
    for j, v in enumerate(SPECIAL):
        put((20 + j) * pk.RUN + (j * 37) % pk.RUN, [v])
    put(5 * pk.RUN, [0] * (2 * pk.RUN))
    put(9 * pk.RUN, [200] * 255 + [0] + [200] * 256)
    put(12 * pk.RUN, [40] * 100 + [0] + [40] * 411)
    put(N - 3, [0, 1000, 0])
    b = var_batch(oracle, bpk=bpk, seed=11, lens=lens, fixed=fixed)
    assert np.array_equal(b.lens[fixed], lens[fixed])
    assert np.unique(b.data[:b.total]).size == 256  # every byte value, so every byte >= 0x80
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    run_var(dev, ab, b)
    assert lines(capfd) == [("binned", "var")]


# ---------------------------------------------------------------- 3 past the staging
def test_past_the_staging(dev, ab, oracle, knobs, capfd):
    """Runs of 512 keys of 100-200 B (about 75 KiB against 24 KiB of staging:
    the later keys are hashed from global memory), and keys of 65 535, 65 536
    and 70 001 bytes -- the batch's first key, one inside, its last -- in
    otherwise short runs."""
    rng = np.random.default_rng(3)
    lens = pk.zipf_lengths(oracle, N, 13)
    fixed = np.zeros(N, bool)
    lens[10 * pk.RUN:20 * pk.RUN] = rng.integers(100, 201, 10 * pk.RUN)
    lens[0], lens[5000], lens[N - 1] = 65_535, 65_536, 70_001
    lens[300], lens[5300] = 65_536, 65_535  # (and past the first one of their runs)
    fixed[10 * pk.RUN:20 * pk.RUN] = True
    fixed[[0, 300, 5000, 5300, N - 1]] = True
    b = var_batch(oracle, seed=13, lens=lens, fixed=fixed)
    assert b.lens[0] == 65_535 and b.lens[N - 1] == 70_001
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    run_var(dev, ab, b)
    assert lines(capfd) == [("binned", "var")]


# ---------------------------------------------------------------- 4 placement
def _call(ab, keys_ptr, off_ptr, n, stride, fid_ptr, F, arena, boff, bpk, out_ptr, ws_ptr, wsb):
    return ab.lib().adl_bloom_probe_batch_device(keys_ptr, off_ptr, n, stride, fid_ptr, F, arena.data_ptr(),
                                                 boff.data_ptr(), None, bpk, out_ptr, ws_ptr, wsb, ab._stream())


@pytest.mark.parametrize("off0", [0, 12_345])
@pytest.mark.parametrize("skew", [0, 1, 7, 15])
def test_placement(dev, ab, knobs, base, skew, off0):
    """Key bytes at any base address and any first offset, inside 0xFF poison;
    offsets inside 0xFF; the answers into a guarded output at skew 3; a
    workspace of exactly workspace_bytes inside guard bands, pre-filled 0xA5
    and then 0x00, with the same answers."""
    knobs.set(KNOB, 1)
    flt = base.flt
    raw = np.concatenate([np.full(off0, 0xFF, np.uint8), base.data[:base.total]])
    dk, doff, dfid = Poisoned(raw, 16, skew=skew), Poisoned(base.off + np.uint64(off0), 8), Poisoned(base.fid, 4)
    assert dk.ptr % 16 == skew
    arena, boff = _d(dev, flt.arena), _d(dev, flt.off)
    wsb = ab.lib().adl_bloom_probe_batch_workspace_bytes(N, flt.F, flt.bpk, 0)
    assert wsb > 256
    answers = []
    for fill in (0xA5, 0x00):
        ws = Guarded(wsb, 256, name="d_workspace")
        ws.view.fill_(fill)
        out = Guarded(N, 8, skew=3, name="d_out")
        rc = _call(ab, dk.ptr, doff.ptr, N, 0, dfid.ptr, flt.F, arena, boff, flt.bpk, out.ptr, ws.ptr, wsb)
        assert rc == 0, rc
        dev.cuda.synchronize()
        got = out.numpy()
        same(got, base.want, f"workspace fill {fill:#x}")
        check_all(out, ws)
        assert not bool((ws.view == fill).all())  # the binned pipeline ran: the direct kernel has no workspace
        answers.append(got.tobytes())
    assert answers[0] == answers[1]


@pytest.mark.parametrize("shape", ["var", "stride 24"])
def test_short_workspace(dev, ab, oracle, knobs, base, shape):
    """A workspace one 256-byte unit short: ADL_ERR_WORKSPACE, nothing written."""
    knobs.set(KNOB, 1)
    b = base if shape == "var" else stride_batch(oracle, 24)
    stride = 0 if shape == "var" else 24
    dk, dfid = _d(dev, b.data), _d(dev, b.fid)
    doff = _d(dev, b.off) if shape == "var" else None
    arena, boff = _d(dev, b.flt.arena), _d(dev, b.flt.off)
    wsb = ab.lib().adl_bloom_probe_batch_workspace_bytes(N, b.flt.F, b.flt.bpk, stride)
    assert wsb > 512
    ws = Guarded(wsb - 256, 256, name="d_workspace")
    out = Guarded(N, 8, skew=3, name="d_out")
    rc = _call(ab, dk.data_ptr(), None if doff is None else doff.data_ptr(), N, stride, dfid.data_ptr(), b.flt.F, arena,
               boff, b.flt.bpk, out.ptr, ws.ptr, wsb - 256)
    assert rc == ADL_ERR_WORKSPACE, rc
    dev.cuda.synchronize()
    check_all(out, ws)
    assert bool((out.view == out.fill).all()) and bool((ws.view == ws.fill).all())


# ---------------------------------------------------------------- 5 fixed strides
@pytest.mark.parametrize("align", [0, 3])
@pytest.mark.parametrize("stride", [1, 4, 15, 17, 24, 48, 49, 64, 100])
def test_fixed_strides(dev, ab, oracle, knobs, capfd, stride, align):
    """Stride 49 is the first whose run of 512 keys exceeds the staging (the
    later keys of each run come from global memory); stride 1 has 256 distinct
    keys, so every run is repeats of a few hash pairs."""
    b = stride_batch(oracle, stride)
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    run_stride(dev, ab, b, align=align)
    assert lines(capfd) == [("binned", f"stride {stride}")]


def test_stride_16_unaligned_is_direct(dev, ab, oracle, knobs, capfd):
    b = stride_batch(oracle, 16)
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    run_stride(dev, ab, b, align=3)
    assert lines(capfd) == [("direct", "stride 16")]


# ---------------------------------------------------------------- 6 order
def test_order(dev, ab, oracle, knobs, capfd):
    """One filter, a random length 0..60 per key, half the keys members: the
    answers as a vector.  Every key of 4 bytes or more carries its index, so
    those are distinct (the 2^20 keys of 0..3 bytes cannot all be).  A pair
    stored at its sorted slot instead of its query's index would give the
    answers in each run's length order: checked first, on the CPU, that this
    order changes the oracle's answers in every run."""
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 61, N)
    off = pk.offsets_of(lens)
    total = int(off[-1])
    data = rng.integers(0, 256, total + 16, dtype=np.uint8)
    idx = np.nonzero(lens >= 4)[0]
    data[pk.ragged(off[idx].astype(np.int64), np.full(idx.size, 4))] = idx.astype("<u4").view(np.uint8)
    member = rng.random(N) < 0.5
    sel = np.nonzero(member)[0]
    mdata = data[pk.ragged(off[sel].astype(np.int64), lens[sel])]
    bm = oracle.keys2block(np.concatenate([mdata, np.zeros(16, np.uint8)]), pk.offsets_of(lens[sel]))

    class One:
        F, bpk, arena, off = 1, 10, np.concatenate([bm, np.zeros(16, np.uint8)]), np.array([0, bm.size], np.uint64)

    fid = np.zeros(N, np.uint32)
    want = oracle.probe_multi(data, fid, One.arena, One.off, offsets=off)
    assert want[member].all() and not want[~member].all()
    assert pk.length_sort_changes_every_run(want, lens)
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    got = ab.probe_batch(_d(dev, data), _d(dev, fid), _d(dev, One.arena), _d(dev, One.off),
                         offsets=_d(dev, off)).cpu().numpy()
    assert lines(capfd) == [("binned", "var")]
    same(got, want, "probe_batch")


# ---------------------------------------------------------------- 7 filters
@pytest.mark.parametrize("F", [1, 4096, 4097])
def test_filter_counts(dev, ab, oracle, knobs, capfd, F):
    """1 filter; 4096, the limit of the LDS histograms; 4097 is direct."""
    sizes = [20_000] if F == 1 else [None if t % 100 == 50 else (t * 37) % 300 for t in range(F)]
    b = var_batch(oracle, seed=70 + F % 7, sizes=sizes)
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    run_var(dev, ab, b)
    assert lines(capfd) == [("binned" if F <= 4096 else "direct", "var")]


def test_filter_ranges_with_gaps(dev, ab, oracle, knobs, capfd):
    """300 filters given by begin / end, in another order with gaps; one of 7
    bytes, one of 0, one of more than one tile (300 000 keys)."""
    sizes = [int(s) for s in np.random.default_rng(300).integers(0, 2000, 300)]
    sizes[7], sizes[11], sizes[100] = 0, None, 300_000
    b = var_batch(oracle, seed=73, sizes=sizes)
    assert b.flt.bms[7].size == 7 and b.flt.bms[11].size == 0 and b.flt.bms[100].size * 8 > 1 << 20
    arena, begin, end = b.flt.scattered()
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    got = ab.probe_batch(_d(dev, b.data), _d(dev, b.fid), _d(dev, arena), _d(dev, begin), offsets=_d(dev, b.off),
                         bitmap_end=_d(dev, end)).cpu().numpy()
    assert lines(capfd) == [("binned", "var")]
    same(got, b.want, "probe_batch")


# ---------------------------------------------------------------- 8 offsets past 2^32
def test_offsets_past_4g(dev, ab, knobs, capfd, base):
    """A device-only key buffer of 2^32 + 2^26 bytes, uninitialised outside the
    window written; offsets start at 2^32 - 150 000."""
    n, first = (1 << 20) + 99, (1 << 32) - 150_000
    total = int(base.off[n])
    assert first + total > (1 << 32) + (1 << 20) and first + total + 64 < BIG_BYTES
    big = dev.empty(BIG_BYTES, dtype=dev.uint8, device="cuda")
    assert big.data_ptr() % 256 == 0
    big[first:first + total] = _d(dev, base.data[:total])
    knobs.set("ADL_BLOOM_DEBUG", 1)
    knobs.set(KNOB, 1)
    capfd.readouterr()
    try:
        run_var(dev, ab, base, n=n, data=big, off=_d(dev, base.off[:n + 1] + np.uint64(first)))
        assert lines(capfd) == [("binned", "var")]
    finally:
        big.untyped_storage().resize_(0)


# ---------------------------------------------------------------- 9 stream
def test_stream_order(dev, ab, knobs, base):
    """On a fresh non-blocking stream behind the delay (tests/streamorder.py):
    the call returns while the delay runs and the answers are exact."""
    knobs.set(KNOB, 1)
    L, flt = ab.lib(), base.flt
    rng = np.random.default_rng(9)
    decoy = rng.integers(0, 256, base.total, dtype=np.uint8)  # the same lengths, other bytes: no members
    decoy_fid = ((base.fid + 1) % (flt.F + 2)).astype(np.uint32)
    wsb = L.adl_bloom_probe_batch_workspace_bytes(N, flt.F, flt.bpk, 0)
    assert wsb > 256, "the binned pipeline's workspace"

    def setup(case):
        keys, fid = case.input(base.data[:base.total], decoy, pad=32), case.input(base.fid, decoy_fid)
        d_off, bm, boff = case.const(base.off), case.const(flt.arena), case.const(flt.off)
        out, ws = case.output(N), case.workspace(wsb)

        def entry(s):
            rc = L.adl_bloom_probe_batch_device(keys.data_ptr(), d_off.data_ptr(), N, 0, fid.data_ptr(), flt.F,
                                                bm.data_ptr(), boff.data_ptr(), None, flt.bpk, out.data_ptr(),
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


# ---------------------------------------------------------------- 10 determinism
def test_same_bytes_twice(dev, ab, knobs, base):
    knobs.set(KNOB, 1)
    d_data, d_off, d_fid = _d(dev, base.data), _d(dev, base.off), _d(dev, base.fid)
    d_arena, d_boff = _d(dev, base.flt.arena), _d(dev, base.flt.off)
    outs = []
    for _ in range(2):
        out = dev.full((N + 64,), 0xA5, dtype=dev.uint8, device="cuda")
        ab.probe_batch(d_data, d_fid, d_arena, d_boff, offsets=d_off, out=out)
        outs.append(out.cpu().numpy().tobytes())
    assert outs[0] == outs[1]
    assert np.array_equal(np.frombuffer(outs[0], np.uint8)[:N], base.want)
