"""GPU: pass B's segment batches (bloom_tile_kernel, adlsm-tree_amd/csrc/
bloom_build.hip) against the oracle, at filters with more chunks than one
batch holds.

A tile's segment descriptors, one per chunk of its filter, are staged in LDS
SEGB at a time: 2048 at one workgroup per CU, 1024 at two.  Past SEGB chunks a
tile takes the `wb > 0` fetch of its table rows, the `nw = min(SEGB, W - wb)`
remainder, the rule that the next tile's rows are prefetched from the last
batch only, and the barrier that frees the segment list for the next batch.
Production plans reach that from about 10 M keys per filter on; here
ADL_BLOOM_CHUNK_KEYS=256 gives a filter of 525 000 keys 2049
chunks, so the seams S-1, S, S+1, ... 3S+1 and the orders around empty and
1-key filters are swept at a few million keys (tests/passbshapes.py).  Three
cases with no knob anchor the sweep to plans a caller gets.

Every case builds through Builder or SegmentedBuilder into a workspace full of
0x5A and a bitmap buffer full of 0xFF, compares every filter byte for byte
with oracle.keys2block (BloomFilter::Keys2Block, reference
src/filter_block.cpp:9-33), and asserts the `adl_bloom plan:` and `adl_bloom
launch:` lines of ADL_BLOOM_DEBUG=1: C, the chunks, the tile size, claim or
dense, the pass-B kernel, and with them the number of batches.  A shape that
stopped reaching a second batch would fail, not pass.
tests/test_pass_b_batches_cpu.py checks each filter's chunk count from C.

The pass-B kernel of each case (D = segments per pipeline stage: 8 at one
workgroup per CU, 4 at two; descriptors from the kernargs or the device
FilterTable, DT; tiles in the static order or from the work queues) and the
batches of its largest filter:

  case                          pass A                    pass B kernel             batches
  sweep[K1..K4-static]          bin16 Src16 dense         D8 kernarg static         3, 2, 4, 3
  sweep[K1..K4-queued]          bin16 Src16 dense queued  D8 kernarg queued         3, 2, 4, 3
  sweep[D1, D2-static]          bin16 Src16 dense         D8 DT static              3, 4
  sweep[D1, D2-queued]          bin16 Src16 dense queued  D8 DT queued              3, 4
  claim[C1], [C1-tight]         bin16 Src16 claim         D8 kernarg static         3 (table entry start << 16 | length)
  sources[var]                  bin16 SrcH dense          D8 kernarg static         3
  sources[var-shifted]          generic bloom_bin_kernel  D8 kernarg static         3
  sources[bpk44], [stride24]    generic bloom_bin_kernel  D8 kernarg static         3
  two_per_cu[M8-static/queued]  generic bloom_bin_kernel  D4 kernarg static/queued  3
  two_per_cu[M16-static/queued] generic bloom_bin_kernel  D4 DT static/queued       4
  two_per_cu_single[B1023..B9M] generic bloom_bin_kernel  D4 kernarg static         1, 1, 2, 3, 4, 2
  production[P2048, P2303]      bin16 Src16 dense         D8 kernarg static         1 (full), 2
  production[P2049+1023]        generic bloom_bin_kernel  D8 kernarg static         2
  repeats[K2, D1, M8, M16 x static, queued]               all eight                 2, 3, 3, 4; three builds each

A bpk-0 filter is one 56-bit tile, so one filter is one pass-B workgroup: a
grid of 1 is no multiple of 8 and keeps the static order under
ADL_BLOOM_BUILD_QUEUES=3 too, which two_per_cu_single asserts; the queued
two-per-CU kernels run in M8 and M16 (8 and 16 tiles).  Random keys would set
each of the 56 bits thousands of times, and the bytes would stay right with
any segment lost; the bpk-0 keys are chosen so that each chunk sets one bit,
the chunks at a batch boundary a bit of their own (_marked below).

Seconds per case on an MI355X, the oracle included where the case is the first
to use its shape (45 cases, 9 s in all): production P2303 1.8, P2048 1.5,
P2049+1023 1.1; sources bpk44 0.5, var 0.2, stride24 0.13, var-shifted 0.04;
sweep K1 0.29, D2 0.27, K4 0.18, D1 0.16, K3 0.09, K2 0.06 static and 0.01 to
0.03 queued; two_per_cu_single B9M 0.26, the others 0.02 or less; claim 0.10
and 0.13; two_per_cu M16 0.09, M8 0.04 static, below 0.01 queued; repeats
0.06 or less.

What the cases notice was tried once with a pass B that dropped the first
segment of every batch after the first (a length of 0 for table entry wb): all
40 cases of more than one batch failed, the 5 of one batch (B1023, B1024,
P2048) passed.
"""
import re

import numpy as np
import pytest

from passbshapes import SHAPES

pytestmark = pytest.mark.gpu

PLAN = re.compile(r"adl_bloom plan: filters (\d+), tile 2\^(\d+) bits, tiles \d+, C (\d+), chunks (\d+), "
                  r"region \d+ words( \(claim\))?, pass B (\d) per CU")
LAUNCH = re.compile(r"adl_bloom launch: pass A (queued|static) \((.+?), (DT|kernarg)\), "
                    r"pass B (queued|static) \((\d) per CU, (DT|kernarg)\)")
GENERIC = "generic bloom_bin_kernel"
ORDERS = ["static", "queued"]


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


# ---------------------------------------------------------------- inputs, references (computed once)
_REF = {}


def _inputs(oracle, name):
    """(host keys, host offsets or None, the oracle's bitmap per filter) of a
    shape.  The production shapes are used once each and not kept."""
    if name in _REF:
        return _REF[name]
    sh = SHAPES[name]
    kb = np.concatenate([[0], np.cumsum(sh.sizes)]).astype(np.int64)
    n = int(kb[-1])
    if sh.keys == "var":
        raw, offs = oracle.synth_varlen(n, seed=0xBA7C4)
        data = np.zeros((int(offs[-1]) + 15) // 16 * 16 + 32, dtype=np.uint8)  # slack for pass A's 16-byte loads
        data[: int(offs[-1])] = raw[: int(offs[-1])]
        want = [oracle.keys2block(data[int(offs[a]):], offs[a:b + 1] - offs[a], bits_per_key=sh.bpk)
                for a, b in zip(kb[:-1], kb[1:])]
        ref = (data, offs, want)
    elif sh.keys == "marked":
        hk = _marked(oracle, sh)
        want = [oracle.keys2block(hk[a:b], bits_per_key=sh.bpk) for a, b in zip(kb[:-1], kb[1:])]
        assert all(0 < np.unpackbits(w).sum() < 56 for w, n_f in zip(want, sh.sizes) if n_f)  # not saturated
        ref = (hk, None, want)
    else:
        if sh.keys == "s24":
            hk = np.random.default_rng(24).integers(0, 256, (n, 24), dtype=np.uint8)
        else:
            hk = oracle.splitmix_keys16(0xBA7C4 + len(sh.sizes), n)
        want = [oracle.keys2block(hk[a:b], bits_per_key=sh.bpk) for a, b in zip(kb[:-1], kb[1:])]
        ref = (hk, None, want)
    if not name.startswith("P"):
        _REF[name] = ref
    return ref


def _marked(oracle, sh):
    """16-byte keys for a bpk-0 build that notices a lost or a foreign segment.
    A bpk-0 bitmap has 56 bits and k = 1 (bit = h1 % 56), so random keys set
    every bit many times over and the bytes stay right whatever pass B drops.
    Here every key of a chunk sets the same bit: bit f % 16 in filter f, and
    a bit of its own (16..55) in the chunks on either side of every batch
    boundary, the first and the last chunk.  A chunk's 256 keys are one bucket
    of a small pool, repeated (repeated keys are legal input)."""
    pool = oracle.splitmix_keys16(0x56B17, 56 * 256 * 4)
    bit = oracle.murmur3_batch(pool)[:, 0] % 56
    bucket = np.stack([pool[bit == b][:256] for b in range(56)])  # (56, 256, 16)
    segb = 2048 if sh.occ == 1 else 1024
    parts = []
    for f, (n, w) in enumerate(zip(sh.sizes, sh.chunks)):
        chunk_bit = np.full(max(w, 1), f % 16, dtype=np.int64)
        marks = sorted({0, w - 1} | {j for e in range(segb, w, segb) for j in (e - 1, e, e + 1) if j < w}) if w else []
        assert len(marks) <= 40
        for i, j in enumerate(marks):
            chunk_bit[j] = 16 + (f * 11 + i) % 40
        i = np.arange(n)
        parts.append(bucket[chunk_bit[i // sh.C], i % 256])
    return np.ascontiguousarray(np.concatenate(parts))


def _run(dev, ab, oracle, knobs, capfd, name, order, a_kernel, builds=1, shift=0, b_order=None):
    """Builds the shape `builds` times into the same dirty buffers; checks the
    bytes of every build and the plan and launch lines.  order: what
    ADL_BLOOM_BUILD_QUEUES asks for; b_order: what pass B has to report."""
    sh = SHAPES[name]
    for k, v in sh.env.items():
        knobs.set(k, v)
    knobs.set("ADL_BLOOM_BUILD_QUEUES", "3" if order == "queued" else "0")
    knobs.set("ADL_BLOOM_DEBUG", "1")
    hk, offs, want = _inputs(oracle, name)
    if shift:  # the key buffer off its 16-byte alignment
        buf = dev.zeros(hk.size + 16 + shift, dtype=dev.uint8, device="cuda")
        buf[shift:shift + hk.size] = dev.from_numpy(hk).cuda()
        keys = buf[shift:]
    else:
        keys = dev.from_numpy(hk).cuda()
    assert keys.data_ptr() % 16 == shift
    doffs = None if offs is None else dev.from_numpy(offs.view(np.int64)).cuda()
    capfd.readouterr()
    if len(sh.sizes) == 1:
        b = ab.Builder(sh.sizes[0], sh.bpk)
        out, boff, nbytes = b.bitmap, [0], [b.nbytes]
    else:
        b = ab.SegmentedBuilder(np.concatenate([[0], np.cumsum(sh.sizes)]), sh.bpk)
        out, boff, nbytes = b.out, b.boff, b.sizes
    b.ws.fill_(0x5A)
    out.fill_(0xFF)
    for r in range(builds):
        b.build(keys, doffs)
        got = out.cpu().numpy()  # (synchronises with the build's stream)
        for f, w in enumerate(want):
            assert int(nbytes[f]) == w.size
            g = got[int(boff[f]):int(boff[f]) + w.size]
            assert np.array_equal(g, w), f"build {r}, filter {f} of {len(want)} ({sh.chunks[f]} chunks): " \
                                         f"{int((g != w).sum())} bytes differ, the first at {int(np.argmax(g != w))}"
    err = capfd.readouterr().err
    # the plan: once for the workspace size, once per build; the same every time
    plans = set(PLAN.findall(err))
    assert plans == {(str(len(sh.sizes)), str(sh.tl), str(sh.C), str(sum(sh.chunks)), " (claim)" if sh.claim else "",
                      str(sh.occ))}, err[-2000:]
    d = "DT" if sh.dt else "kernarg"
    a_order = "queued" if order == "queued" and a_kernel != GENERIC else "static"
    line = (a_order, a_kernel, d, b_order or order, str(sh.occ), d)
    assert [m.groups() for m in LAUNCH.finditer(err)] == [line] * builds


# ---------------------------------------------------------------- a. the chunk-count sweep
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["K1", "K2", "K3", "K4", "D1", "D2"])
def test_sweep(dev, ab, oracle, knobs, capfd, name, order):
    """16-byte keys, bpk 10, 256 keys per chunk: filters of 1, 15, 16, 17, 255,
    256, 257, S-1, S, S+1, S+15, S+16, S+17, 2S-1, 2S, 2S+1, 2S+17 and 3S+1
    chunks (S = 2048) side by side, so adjacent tiles belong to filters of
    different W; an empty and a 1-key filter between two multi-batch filters
    in both orders (the W == 0 prefetch, and the prefetch of the next tile's
    rows from the last batch only).  K: up to 8 filters, D: more."""
    assert SHAPES[name].batches >= 2
    _run(dev, ab, oracle, knobs, capfd, name, order, "bin16 Src16 dense")


# ---------------------------------------------------------------- b. the claim layout
@pytest.mark.parametrize("name", ["C1", "C1-tight"])
def test_claim(dev, ab, oracle, knobs, capfd, name):
    """ADL_BLOOM_CLAIM=2: the table entry is (start << 16) | length, one word
    per (tile, chunk), at S-1, S, S+1 and 2S+1 chunks; tight: the region capped
    at 101 % of k*C with 2^20-bit tiles (a share of 16 slots for a mean run of
    19), so most chunks overflow and are sorted exactly."""
    _run(dev, ab, oracle, knobs, capfd, name, "static", "bin16 Src16 claim")


# ---------------------------------------------------------------- c. other pass-A sources
def test_sources_varlen(dev, ab, oracle, knobs, capfd):
    """Keys of 8-256 bytes in an aligned buffer: the hashing pass, then pass A
    over the (h1, h2) pairs; S+1 and 2S+1 chunks."""
    _run(dev, ab, oracle, knobs, capfd, "var", "static", "bin16 SrcH dense")


def test_sources_varlen_shifted(dev, ab, oracle, knobs, capfd):
    """The same keys one byte off the alignment: the generic pass A."""
    _run(dev, ab, oracle, knobs, capfd, "var", "static", GENERIC, shift=1)


@pytest.mark.parametrize("name", ["bpk44", "stride24"])
def test_sources_generic(dev, ab, oracle, knobs, capfd, name):
    """bpk 44 (k = 30: 7680 positions per chunk region) and keys of 24 bytes."""
    _run(dev, ab, oracle, knobs, capfd, name, "static", GENERIC)


# ---------------------------------------------------------------- d. two workgroups per CU
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["M8", "M16"])
def test_two_per_cu(dev, ab, oracle, knobs, capfd, name, order):
    """bpk 0: k = 1 and every filter is one 56-bit tile, so the plan runs two
    pass-B workgroups per CU with batches of 1024.  Filters of 1023, 1024,
    1025, 1040, 2049 and 3073 chunks, an empty and a 1-key filter between;
    every position of a chunk falls into the one tile, so every segment is
    256 long (the long-segment loop).  Keys: _marked."""
    assert SHAPES[name].occ == 2 and SHAPES[name].batches >= 3
    _run(dev, ab, oracle, knobs, capfd, name, order, GENERIC)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["B1023", "B1024", "B1261", "B2301", "B3278", "B9M"])
def test_two_per_cu_single(dev, ab, oracle, knobs, capfd, name, order):
    """One bpk-0 filter: one workgroup walks every batch of the one tile.  With
    the knob 1023 and 1024 chunks (one batch), 1261, 2301 and 3278 (two to
    four); with no knob 9 M keys in 1280 chunks of 7032 keys, segments of 7032
    positions.  A grid of one workgroup keeps the static order whatever
    ADL_BLOOM_BUILD_QUEUES says."""
    sh = SHAPES[name]
    assert sh.occ == 2 and sh.batches == {"B1023": 1, "B1024": 1, "B1261": 2, "B2301": 3, "B3278": 4, "B9M": 2}[name]
    _run(dev, ab, oracle, knobs, capfd, name, order, GENERIC, b_order="static")


# ---------------------------------------------------------------- e. production plans
@pytest.mark.parametrize("name", ["P2048", "P2303", "P2049+1023"])
def test_production(dev, ab, oracle, knobs, capfd, name):
    """No knob: 10 013 958 keys plan exactly 2048 chunks (one full batch, and
    the next tile's rows prefetched from it), 12 M keys 2303 (a second batch
    of 255), and 2 458 200 + 1 227 000 keys at bpk 44 plan 2049 + 1023 (a
    second batch of one segment: 15 of 16 waves idle)."""
    assert not SHAPES[name].env
    knobs.unset("ADL_BLOOM_CHUNK_KEYS")
    _run(dev, ab, oracle, knobs, capfd, name, "static", GENERIC if SHAPES[name].bpk == 44 else "bin16 Src16 dense")


# ---------------------------------------------------------------- f. build after build
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["K2", "D1", "M8", "M16"])
def test_repeats(dev, ab, oracle, knobs, capfd, name, order):
    """Three builds into the same dirty workspace and bitmaps, one multi-batch
    shape per pass-B kernel: D 8 / 4 x kernarg / DT x static / queued."""
    assert SHAPES[name].batches >= 2
    a_kernel = GENERIC if SHAPES[name].bpk == 0 else "bin16 Src16 dense"
    _run(dev, ab, oracle, knobs, capfd, name, order, a_kernel, builds=3)
