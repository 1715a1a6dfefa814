"""GPU: the work-queue forms of the build passes (bloom_bin16_kernel<..., DYN>
and bloom_tile_kernel<..., DYN>, fed by GroupQueue in
adlsm-tree_amd/csrc/bloom_build.hip) against the oracle.

By default a build takes its chunks and tiles from the queues only while a
probe server's kernel is resident and a pass has many items per workgroup, so
no ordinary test reaches these kernels.  ADL_BLOOM_BUILD_QUEUES=3 queues
always: every case here sets it with ADL_BLOOM_DEBUG=1, reads
the `adl_bloom launch:` line of each launch pair from stderr to see which
kernels ran and in which order, and compares every filter byte for byte with
oracle.keys2block (BloomFilter::Keys2Block, reference src/filter_block.cpp:9-33).
A launch whose grid is no multiple of 8 keeps the static order without an
error, which is why each case asserts the line and not only the bitmap.

The shapes came from a CPU model of make_plan at 256 CUs (the plan line of
adl_bloom_build_workspace_bytes), not from a GPU run; the launch line on the
GPU is the authority.  What each case runs (pass A kernel / descriptors;
pass B workgroups per CU) and what the line said on an MI355X:

  case                                   pass A                        pass B  line on MI355X
  shapes[8x300]                          bin16 Src16 dense, kernarg    2       queued / queued
  shapes[8x300-tl20]                     bin16 Src16 claim, kernarg    1       queued / queued
  shapes[8x300-tl20-dense]               bin16 Src16 dense, kernarg    1       queued / queued
  shapes[8x300-tight, 8x2000-tight]      bin16 Src16 claim (overflow)  2, 1    queued / queued
  shapes[...-tight-tl20]                 bin16 Src16 claim (overflow)  1       queued / queued
  shapes[empties, empties-tl20]          dense / claim, kernarg        1       queued / queued
  shapes[304x300]                        bin16 Src16 claim, DT         2       queued / queued
  shapes[304x300-dense]                  bin16 Src16 dense, DT         2       queued / queued
  shapes[304x300-tl20]                   bin16 Src16 claim, DT         1       queued / queued
  shapes[304x300-tl20-dense]             bin16 Src16 dense, DT         1       queued / queued
  shapes[mixed14]                        bin16 Src16 dense, DT         1       queued / queued
  shapes[1x100000, 1x4096]               bin16 Src16 dense, kernarg    1       queued / queued
  varlen[8x300-claim / -dense]           bin16 SrcH claim / dense, kernarg  2  queued / queued
  varlen[304x300-claim / -dense]         bin16 SrcH claim / dense, DT  2       queued / queued
  varlen[mixed14-claim / -dense]         bin16 SrcH claim / dense, DT  1       queued / queued
  varlen_unaligned                       generic bloom_bin_kernel      2       static / queued
  other_k[bpk 1, 3, 20, 44], stride24    generic bloom_bin_kernel      2, 1    static / queued
  skip_adjacent_duplicates               generic bloom_bin_kernel, DT  2       static / queued
  repeated_hash_table[8 / 304 filters]   bin16 Src16 dense / claim     2       queued / queued
  queue_passes[1], [2]                   as shapes[8x300], [304x300]   2       queued / static, static / queued
  dirty_buffers                          as shapes[1x100000], [304x300]        queued / queued, three builds each
  queued_equals_static                   ADL_BLOOM_BUILD_QUEUES=0              static / static, the same bytes
  host_entry                             bin16 Src16 dense, DT         1       queued / queued

So the eight queued pass-A kernels (Src16 / SrcH x kernarg / DT x dense /
claim) and the four queued pass-B kernels (1 / 2 per CU x kernarg / DT) each
run in at least one case.  No shape of the model had to be replaced.
"""
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"adl_bloom launch: pass A (queued|static) \((.+?), (DT|kernarg)\), "
                    r"pass B (queued|static) \((\d) per CU, (DT|kernarg)\)")

S8 = [300] * 8
S304 = [300] * 304  # 304 chunks over 256 workgroups: the second round leaves groups 2-7 dry
EMPTIES = [300, 0, 1, 1625, 0, 300, 257, 300]
EMPTIES_TL20 = [300, 0, 1, 1537, 0, 300, 257, 300]
MIXED14 = [0, 1, 511, 512, 513, 1025, 0, 1, 769, 3, 700, 12, 4096, 1]
TL20 = {"ADL_BLOOM_TILE_LOG2": "20"}
DENSE = {"ADL_BLOOM_CLAIM": "0"}
TIGHT = {"ADL_BLOOM_CLAIM": "2", "ADL_BLOOM_CLAIM_CAP": "101"}  # most chunks overflow their tiles' shares


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def ab():
    import adlbloom

    adlbloom.lib()
    return adlbloom


@pytest.fixture
def queued(knobs):
    knobs.set("ADL_BLOOM_BUILD_QUEUES", "3")
    knobs.set("ADL_BLOOM_DEBUG", "1")
    return knobs


def _set(knobs, *dicts):
    for d in dicts:
        for k, v in d.items():
            knobs.set(k, v)


def _launches(capfd):
    """The launch lines printed since the last call, as tuples
    (A order, A kernel, A descriptors, B order, B per CU, B descriptors)."""
    return [m.groups() for m in LAUNCH.finditer(capfd.readouterr().err)]


def _line(a, kernel, b, occ, dt):
    d = "DT" if dt else "kernarg"
    return (a, kernel, d, b, str(occ), d)


# ---------------------------------------------------------------- inputs, references (computed once)
_REF = {}


def _kb(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _fixed(oracle, sizes, bpk=10, stride=16):
    """(key_begin, host keys (n, stride), the oracle's bitmap per filter)."""
    key = ("fixed", tuple(sizes), bpk, stride)
    if key not in _REF:
        kb = _kb(sizes)
        n = int(kb[-1])
        if stride == 16:
            hk = oracle.splitmix_keys16(0xB10C + len(sizes), n)
        else:
            hk = np.random.default_rng(stride).integers(0, 256, (n, stride), dtype=np.uint8)
        want = [oracle.keys2block(hk[int(kb[f]):int(kb[f + 1])], bits_per_key=bpk) for f in range(len(sizes))]
        _REF[key] = (kb, hk, want)
    return _REF[key]


def _same(oracle, nf, n=300):
    """nf filters that all hold the same n SplitMix keys."""
    key = ("same", nf, n)
    if key not in _REF:
        base = oracle.splitmix_keys16(0x5A4E, n)
        h = oracle.murmur3_batch(base)
        # the point of the case: many keys whose two hashes are equal
        assert (h[:, 0] == h[:, 1]).sum() > n // 4
        want = oracle.keys2block(base)
        _REF[key] = (_kb([n] * nf), np.tile(base, (nf, 1)), [want] * nf)
    return _REF[key]


def _varlen(oracle, sizes):
    """Keys of 0-120 random bytes: (key_begin, packed bytes in a buffer with
    16 bytes of slack, offsets, the oracle's bitmap per filter)."""
    key = ("var", tuple(sizes))
    if key not in _REF:
        kb = _kb(sizes)
        rng = random.Random(1000 + len(sizes))
        keys = [rng.randbytes(rng.randrange(0, 121)) for _ in range(int(kb[-1]))]
        data, offs = oracle.pack(keys)
        pad = np.zeros(((data.size + 15) // 16) * 16 + 32, dtype=np.uint8)
        pad[: data.size] = data
        want = [oracle.keys2block(keys[int(kb[f]):int(kb[f + 1])]) for f in range(len(sizes))]
        _REF[key] = (kb, pad, offs, want)
    return _REF[key]


def _check(out, boff, nbytes, want):
    out = out.cpu().numpy()
    for f, w in enumerate(want):
        got = out[int(boff[f]):int(boff[f]) + int(nbytes[f])]
        assert np.array_equal(got, w), f"filter {f} of {len(want)}"


def _build_fixed(dev, ab, kb, hk, want, bpk=10, flags=0):
    """One filter through ab.build, more through ab.build_segmented; checked."""
    keys = dev.from_numpy(hk).cuda()
    if len(want) == 1:
        got = ab.build(keys, bits_per_key=bpk).cpu().numpy()
        assert np.array_equal(got, want[0])
        return got
    out, boff, nbytes = ab.build_segmented(keys, kb, bits_per_key=bpk, flags=flags)
    _check(out, boff, nbytes, want)
    return out.cpu().numpy()


# ---------------------------------------------------------------- 16-byte keys
@pytest.mark.parametrize("sizes,extra,kernel,occ", [
    (S8, {}, "bin16 Src16 dense", 2),
    (S8, TL20, "bin16 Src16 claim", 1),
    (S8, {**TL20, **DENSE}, "bin16 Src16 dense", 1),
    (S8, TIGHT, "bin16 Src16 claim", 2),
    (S8, {**TIGHT, **TL20}, "bin16 Src16 claim", 1),
    ([2000] * 8, TIGHT, "bin16 Src16 claim", 1),
    ([2000] * 8, {**TIGHT, **TL20}, "bin16 Src16 claim", 1),
    (EMPTIES, {}, "bin16 Src16 dense", 1),
    (EMPTIES_TL20, TL20, "bin16 Src16 claim", 1),
    (S304, {}, "bin16 Src16 claim", 2),
    (S304, DENSE, "bin16 Src16 dense", 2),
    (S304, TL20, "bin16 Src16 claim", 1),
    (S304, {**TL20, **DENSE}, "bin16 Src16 dense", 1),
    (MIXED14, {}, "bin16 Src16 dense", 1),
    ([100_000], {}, "bin16 Src16 dense", 1),
    ([4096], {}, "bin16 Src16 dense", 1),
], ids=["8x300", "8x300-tl20", "8x300-tl20-dense", "8x300-tight", "8x300-tight-tl20", "8x2000-tight",
        "8x2000-tight-tl20", "empties", "empties-tl20", "304x300", "304x300-dense", "304x300-tl20",
        "304x300-tl20-dense", "mixed14", "1x100000", "1x4096"])
def test_queued_shapes(dev, ab, oracle, queued, capfd, sizes, extra, kernel, occ):
    """Both passes from the queues.  8 x 300: 16 chunks over 16 workgroups that
    each take three ahead, so most steal from other groups and several find
    the queues dry at once; at 2^20-bit tiles, 8 tiles for 8 workgroups.  The
    tight settings make most chunks overflow (the exact sort inside the queued
    claim kernel).  Empty and 1-key filters: pass B's prefetch for a tile with
    no chunk.  304 x 300 and the 14 mixed sizes: descriptors from the device
    FilterTable, a partial last round.  1 x 100 000: 977 tiles over 256
    workgroups, a ragged fourth round."""
    _set(queued, extra)
    kb, hk, want = _fixed(oracle, sizes)
    _build_fixed(dev, ab, kb, hk, want)
    assert _launches(capfd) == [_line("queued", kernel, "queued", occ, len(sizes) > 8)]


# ---------------------------------------------------------------- variable-length keys
@pytest.mark.parametrize("claim", ["claim", "dense"])
@pytest.mark.parametrize("sizes,occ", [(S8, 2), (S304, 2), (MIXED14, 1)], ids=["8x300", "304x300", "mixed14"])
def test_queued_varlen(dev, ab, oracle, queued, capfd, sizes, occ, claim):
    """Keys of 0-120 bytes in a 16-byte-aligned buffer: the hashing pass, then
    the queued pass A over the (h1, h2) pairs (Src = SrcH)."""
    queued.set("ADL_BLOOM_CLAIM", "2" if claim == "claim" else "0")
    kb, pad, offs, want = _varlen(oracle, sizes)
    data = dev.from_numpy(pad).cuda()
    assert data.data_ptr() % 16 == 0
    out, boff, nbytes = ab.build_segmented(data, kb, offsets=dev.from_numpy(offs.view(np.int64)).cuda())
    _check(out, boff, nbytes, want)
    assert _launches(capfd) == [_line("queued", "bin16 SrcH " + claim, "queued", occ, len(sizes) > 8)]


def test_queued_varlen_unaligned(dev, ab, oracle, queued, capfd):
    """The key buffer shifted by one byte: no staged 16-byte loads, so pass A
    is the generic kernel in the static order, and pass B still queues."""
    kb, pad, offs, want = _varlen(oracle, S8)
    buf = dev.zeros(pad.size + 16, dtype=dev.uint8, device="cuda")
    buf[1:1 + pad.size] = dev.from_numpy(pad).cuda()
    data = buf[1:]
    assert data.data_ptr() % 16 == 1
    out, boff, nbytes = ab.build_segmented(data, kb, offsets=dev.from_numpy(offs.view(np.int64)).cuda())
    _check(out, boff, nbytes, want)
    assert _launches(capfd) == [_line("static", "generic bloom_bin_kernel", "queued", 2, False)]


# ---------------------------------------------------------------- generic pass A, queued pass B
def _dirty_segmented(dev, ab, kb, hk, want, bpk, builds):
    sb = ab.SegmentedBuilder(kb, bpk)
    sb.ws.fill_(0x5A)
    sb.out.fill_(0xFF)
    keys = dev.from_numpy(hk).cuda()
    for _ in range(builds):
        out = sb.build(keys)
        dev.cuda.synchronize()
        _check(out, sb.boff, sb.sizes, want)


@pytest.mark.parametrize("bpk", [1, 3, 20, 44])
@pytest.mark.parametrize("sizes", [S8, S304], ids=["8x300", "304x300"])
def test_queued_pass_b_other_k(dev, ab, oracle, queued, capfd, sizes, bpk):
    """k != 6: pass A is the generic kernel (static), pass B takes its tiles
    from the queues; twice into a dirty workspace and bitmap, so the queue
    counters are cleared although pass A does not use them."""
    kb, hk, want = _fixed(oracle, sizes, bpk=bpk)
    _dirty_segmented(dev, ab, kb, hk, want, bpk, 2)
    assert _launches(capfd) == [_line("static", "generic bloom_bin_kernel", "queued", 2, len(sizes) > 8)] * 2


def test_queued_pass_b_stride24(dev, ab, oracle, queued, capfd):
    """30 000 keys of 24 bytes (no 16-byte view): generic pass A, queued pass B."""
    kb, hk, want = _fixed(oracle, [30_000], stride=24)
    b = ab.Builder(30_000, 10)
    b.ws.fill_(0x5A)
    b.bitmap.fill_(0xFF)
    keys = dev.from_numpy(hk).cuda()
    for r in range(2):
        assert np.array_equal(b.build(keys).cpu().numpy(), want[0]), r
    assert _launches(capfd) == [_line("static", "generic bloom_bin_kernel", "queued", 1, False)] * 2


def test_queued_skip_adjacent_duplicates(dev, ab, oracle, queued, capfd):
    """ADL_BLOOM_SKIP_ADJACENT_DUPLICATES needs the keys in order: the generic
    pass A.  304 filters of 150 distinct keys, each twice in a row (300 is
    even, so no pair straddles two filters)."""
    kb, hk, _ = _fixed(oracle, S304)
    hk2 = hk.copy()
    hk2[1::2] = hk2[0::2]
    want2 = [oracle.keys2block(hk2[int(kb[f]):int(kb[f + 1])]) for f in range(len(S304))]
    _build_fixed(dev, ab, kb, hk2, want2, flags=ab.SKIP_ADJACENT_DUPLICATES)
    assert _launches(capfd) == [_line("static", "generic bloom_bin_kernel", "queued", 2, True)]


# ---------------------------------------------------------------- the repeated-hash table
@pytest.mark.parametrize("dedup", ["1", "0"])
@pytest.mark.parametrize("nf,kernel", [(8, "bin16 Src16 dense"), (304, "bin16 Src16 claim")], ids=["8", "304"])
def test_queued_repeated_hash_table_across_filters(dev, ab, oracle, queued, capfd, nf, kernel, dedup):
    """Every filter holds the same 300 SplitMix keys, about 39 % of them with
    h1 == h2 (the keys the repeated-hash table skips).  A workgroup's next
    chunk comes from the queues and may belong to any filter, an earlier one
    too (stealing wraps from group 7 to group 0); a table that survived the
    change of filter would drop the second filter's bits.  Every filter must
    carry every bit."""
    queued.set("ADL_BLOOM_HASH_DEDUP", dedup)
    kb, hk, want = _same(oracle, nf)
    _build_fixed(dev, ab, kb, hk, want)
    assert _launches(capfd) == [_line("queued", kernel, "queued", 2, nf > 8)]


# ---------------------------------------------------------------- one pass queued
@pytest.mark.parametrize("passes", ["1", "2"])
@pytest.mark.parametrize("sizes,kernel", [(S8, "bin16 Src16 dense"), (S304, "bin16 Src16 claim")],
                         ids=["8x300", "304x300"])
def test_queue_passes(dev, ab, oracle, queued, capfd, sizes, kernel, passes):
    """ADL_BLOOM_BUILD_QUEUE_PASSES = 1 queues pass A only, 2 pass B only; the
    bytes equal those with both queued."""
    kb, hk, want = _fixed(oracle, sizes)
    both = _build_fixed(dev, ab, kb, hk, want)
    dt = len(sizes) > 8
    assert _launches(capfd) == [_line("queued", kernel, "queued", 2, dt)]
    queued.set("ADL_BLOOM_BUILD_QUEUE_PASSES", passes)
    one = _build_fixed(dev, ab, kb, hk, want)
    a, b = ("queued", "static") if passes == "1" else ("static", "queued")
    assert _launches(capfd) == [_line(a, kernel, b, 2, dt)]
    assert np.array_equal(one, both)


# ---------------------------------------------------------------- dirty buffers, build after build
def test_dirty_buffers_builder(dev, ab, oracle, queued, capfd):
    """Three builds of 1 x 100 000 into a workspace full of 0x5A and a bitmap
    full of 0xFF: the queue counters are cleared before every launch pair (a
    counter left from the last build, or the fill, hands out no tile, and the
    tile keeps its 0xFF), and every tile is written."""
    kb, hk, want = _fixed(oracle, [100_000])
    b = ab.Builder(100_000, 10)
    b.ws.fill_(0x5A)
    b.bitmap.fill_(0xFF)
    keys = dev.from_numpy(hk).cuda()
    for r in range(3):
        assert np.array_equal(b.build(keys).cpu().numpy(), want[0]), r
    assert _launches(capfd) == [_line("queued", "bin16 Src16 dense", "queued", 1, False)] * 3


def test_dirty_buffers_segmented_builder(dev, ab, oracle, queued, capfd):
    """The same for 304 x 300 through a SegmentedBuilder (claim layout, the
    FilterTable in the dirty workspace, two pass-B workgroups per CU)."""
    kb, hk, want = _fixed(oracle, S304)
    _dirty_segmented(dev, ab, kb, hk, want, 10, 3)
    assert _launches(capfd) == [_line("queued", "bin16 Src16 claim", "queued", 2, True)] * 3


# ---------------------------------------------------------------- queued against static
@pytest.mark.parametrize("sizes,kernel,occ", [
    (S8, "bin16 Src16 dense", 2), (S304, "bin16 Src16 claim", 2), ([100_000], "bin16 Src16 dense", 1),
], ids=["8x300", "304x300", "1x100000"])
def test_queued_equals_static(dev, ab, oracle, queued, capfd, sizes, kernel, occ):
    kb, hk, want = _fixed(oracle, sizes)
    dt = len(sizes) > 8
    q = _build_fixed(dev, ab, kb, hk, want)
    assert _launches(capfd) == [_line("queued", kernel, "queued", occ, dt)]
    queued.set("ADL_BLOOM_BUILD_QUEUES", "0")
    s = _build_fixed(dev, ab, kb, hk, want)
    assert _launches(capfd) == [_line("static", kernel, "static", occ, dt)]
    assert np.array_equal(q, s)


# ---------------------------------------------------------------- host entry
def test_queued_host_entry(dev, ab, oracle, queued, capfd):
    """adl_bloom_build_segmented (host pointers, the pipelined groups: one
    group here) launches the same queued pair."""
    kb, hk, want = _fixed(oracle, MIXED14)
    sizes = np.array([w.size for w in want], dtype=np.uint64)
    boff = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]]).astype(np.uint64)
    out = np.full(int(boff[-1] + sizes[-1]) + 16, 0xFF, dtype=np.uint8)
    ab.build_segmented_host(hk, kb, out, boff)
    for f, w in enumerate(want):
        assert np.array_equal(out[int(boff[f]):int(boff[f]) + w.size], w), f
    assert _launches(capfd) == [_line("queued", "bin16 Src16 dense", "queued", 1, True)]
