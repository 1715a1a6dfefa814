"""GPU: the edges of pass A's chunk loop (bloom_bin16_kernel in
adlsm-tree_amd/csrc/bloom_build.hip), every byte against oracle.keys2block.

What the loop does that these cases aim at:

* the LDS (tile counters, repeated-pair table) is set up before chunk 0's
  keys are waited for and hashed;
* a workgroup prefetches keys two chunks ahead with unconditional, clamped
  loads; past its last chunk (its last two steps, and the prologue's second
  load of a workgroup with one chunk) every lane loads key 0 of the launch's
  last chunk and the result is never hashed into a filter;
* a filter's last chunk clears the repeated-pair table, and the next filter
  may have another T and so other counters and table entries per thread.

Shapes.  ADL_BLOOM_CHUNK_KEYS=256 caps C at 256 keys, so a few hundred
thousand keys give a workgroup up to four chunks.  Every case reads the
plan's line (ADL_BLOOM_DEBUG) for the chunk count W; pass A's grid is G =
min(W, CUs), and every case checks it against the grid its launch line
reports.  make_plan evens the chunks out over whole rounds of the grid, so one
filter of n keys has n / 256 chunks only up to G and at 2G; a single filter
cannot have G + 1, 2G + 1 or 3G + 1 chunks (C shrinks and the second round
fills up).  Those counts are reached with G + 1, 2G + 1 and 3G + 1 filters of
4 keys (C = 4, one chunk each), and the ragged rounds a single filter does
have (n = r * G * 256 + 1: r full rounds and a part of one) stand beside them,
so workgroups with 0, 1, 2, 3 and 4 chunks all occur, within one filter and
across filters.

Every case builds three times into the same workspace and bitmap buffer.
"""
import ctypes
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAN = re.compile(r"adl_bloom plan: filters (\d+), tile 2\^(\d+) bits, tiles (\d+), C (\d+), chunks (\d+), "
                  r"region (\d+) words( \(claim\))?")
LAUNCH = re.compile(r"adl_bloom launch: pass A (queued|static) \((.+?), (DT|kernarg)\), pass B .+?; "
                    r"grids (\d+), (\d+)")
CK = 256  # ADL_BLOOM_CHUNK_KEYS


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


@pytest.fixture(scope="module")
def G(dev):
    """Pass A's grid when the chunks fill it: one workgroup per CU."""
    return dev.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture
def small(knobs):
    knobs.set("ADL_BLOOM_CHUNK_KEYS", str(CK))
    knobs.set("ADL_BLOOM_DEBUG", "1")
    knobs.set("ADL_BLOOM_CLAIM", "0")
    return knobs


def _lines(capfd):
    """(plans, launches) printed since the last call: plans as dicts, launches
    as (order, kernel, descriptors).  Every launch's pass-A grid must be
    min(chunks, CUs): the cases' counts of chunks per workgroup rest on it."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    err = capfd.readouterr().err
    plans = [dict(filters=int(m[1]), TL=int(m[2]), tiles=int(m[3]), C=int(m[4]), chunks=int(m[5]), claim=bool(m[7]))
             for m in PLAN.finditer(err)]
    launches = [m.groups() for m in LAUNCH.finditer(err)]
    assert plans and all(int(l[3]) == min(plans[-1]["chunks"], cus) for l in launches), (plans[-1], launches)
    return plans, [l[:3] for l in launches]


# ---------------------------------------------------------------- inputs and references, computed once
_REF = {}


def _kb(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _want(oracle, hk, kb, bpk):
    return [oracle.keys2block(hk[int(kb[f]):int(kb[f + 1])], bits_per_key=bpk) for f in range(len(kb) - 1)]


def _fixed(oracle, sizes, bpk=10):
    key = ("fixed", tuple(sizes), bpk)
    if key not in _REF:
        kb = _kb(sizes)
        hk = oracle.splitmix_keys16(0xA110 + len(sizes) + int(kb[-1]) % 97, int(kb[-1]))
        _REF[key] = (kb, hk, _want(oracle, hk, kb, bpk))
    return _REF[key]


def _three_builds(dev, ab, kb, keys, want, bpk=10, offsets=None):
    """Three builds into one SegmentedBuilder's workspace and bitmaps, each compared."""
    sb = ab.SegmentedBuilder(kb, bpk)
    for r in range(3):
        out = sb.build(keys, offsets)
        dev.cuda.synchronize()
        got = out.cpu().numpy()
        for f, w in enumerate(want):
            o = int(sb.boff[f])
            assert np.array_equal(got[o:o + int(sb.sizes[f])], w), f"build {r}, filter {f} of {len(want)}"


def _run_fixed(dev, ab, oracle, capfd, sizes, bpk=10):
    kb, hk, want = _fixed(oracle, sizes, bpk)
    capfd.readouterr()
    _three_builds(dev, ab, kb, dev.from_numpy(hk).cuda(), want, bpk)
    return _lines(capfd)


def _dense16(launches, order="static"):
    assert launches and all(l[0] == order and l[1] == "bin16 Src16 dense" for l in launches), launches


# ---------------------------------------------------------------- chunk counts per launch
@pytest.mark.parametrize("chunks", ["1", "2", "3", "G-1", "G", "2G"])
def test_chunk_counts_one_filter(dev, ab, oracle, small, capfd, G, chunks):
    """W = 1, 2, 3 (a grid of W workgroups with one chunk each: the prologue's
    second load and every refill are clamped to the last chunk), G - 1, G
    (one full round) and 2G (two: the refill of the last step is clamped)."""
    W = {"1": 1, "2": 2, "3": 3, "G-1": G - 1, "G": G, "2G": 2 * G}[chunks]
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [W * CK])
    assert plans[-1]["chunks"] == W and plans[-1]["C"] == CK and not plans[-1]["claim"]
    _dense16(launches)


@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_chunk_counts_tiny_filters(dev, ab, oracle, small, capfd, G, rounds):
    """G + 1, 2G + 1 and 3G + 1 chunks: that many filters of 4 keys.  Workgroup
    0 has one chunk more than the others (2 against 1, ..., 4 against 3), and
    every chunk is its filter's last, so the repeated-pair table is cleared at
    every step."""
    W = rounds * G + 1
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [4] * W)
    assert plans[-1]["chunks"] == W and plans[-1]["C"] == 4
    _dense16(launches)


@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_ragged_rounds_one_filter(dev, ab, oracle, small, capfd, G, rounds):
    """n = rounds * G * 256 + 1 keys of one filter: rounds full rounds and a
    part of another, all in one filter (1 and 2, 2 and 3, 3 and 4 chunks per
    workgroup): the workgroups that stop a round early run their last two
    steps, with the one-key loads past the end, while the others still load
    whole chunks."""
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [rounds * G * CK + 1])
    W = plans[-1]["chunks"]
    assert rounds * G < W <= (rounds + 1) * G and W % G != 0, plans[-1]
    _dense16(launches)


# ---------------------------------------------------------------- chunk sizes
@pytest.mark.parametrize("last", [1, CK - 1, CK])
@pytest.mark.parametrize("full", ["3", "2G-1"])
def test_last_chunk_size(dev, ab, oracle, small, capfd, G, last, full):
    """A last chunk of 1 key, of C - 1 keys and of exactly C keys, behind 3
    full chunks (one per workgroup) and behind 2G - 1 (the second chunk of the
    last workgroup)."""
    F = 3 if full == "3" else 2 * G - 1
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [F * CK + last])
    assert plans[-1]["chunks"] == F + 1 and plans[-1]["C"] == CK
    _dense16(launches)


# ---------------------------------------------------------------- filter boundaries
BOUNDARIES = {
    # two filters, the boundary inside round 0: the workgroups of filter 0's chunks meet filter 1 in their next step
    "2-filters": [40_000, 50_000],
    # three filters of different T, the middle one of one chunk
    "1-chunk-between": [30_000, 100, 60_000],
    # four to five chunks per workgroup, boundaries in rounds 1, 1 and 3
    "4-filters": [100_000, 150, 120_000, 70_000],
    # three equal filters over four rounds: each boundary at another place of its round
    "3-long": [66_300, 66_300, 66_300],
}


@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_filter_boundaries(dev, ab, oracle, small, capfd, G, name):
    """Several filters in one launch: at a filter's last chunk the
    repeated-pair table is cleared, and T, m and with them the counters a
    thread scans change from one step of a workgroup to the next."""
    sizes = BOUNDARIES[name]
    plans, launches = _run_fixed(dev, ab, oracle, capfd, sizes)
    p = plans[-1]
    assert p["filters"] == len(sizes) and p["chunks"] > G and not p["claim"], p
    per = [-(-s // p["C"]) for s in sizes]
    assert sum(per) == p["chunks"]
    assert any(c % G for c in np.cumsum(per)[:-1]), "a boundary inside a round"
    if name == "1-chunk-between":
        assert per[1] == 1
    _dense16(launches)


@pytest.mark.parametrize("n,tl,tiles", [(131_072, 13, 1281), (838_860, 15, 2048)], ids=["T1281", "T2048"])
def test_counters_two_and_three_per_thread(dev, ab, oracle, small, capfd, n, tl, tiles):
    """More than 1024 tiles (ADL_BLOOM_TILE_LOG2=13 asks for the smallest
    tiles the plan grants): a thread scans two counters and stores two table
    entries per chunk; at T = 2048, the most a filter can have, three."""
    small.set("ADL_BLOOM_TILE_LOG2", "13")
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [n])
    assert plans[-1]["TL"] == tl and plans[-1]["tiles"] == tiles, plans[-1]
    _dense16(launches)


def test_tiles_change_across_filters(dev, ab, oracle, small, capfd, G):
    """Filters of 2048 tiles, of one tile and of 321 in one launch: three, one
    and one counters per thread from filter to filter."""
    small.set("ADL_BLOOM_TILE_LOG2", "13")
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [838_860, 7, 131_072])
    assert plans[-1]["chunks"] > 2 * G
    assert plans[-1]["TL"] == 15 and plans[-1]["tiles"] == 2048 + 1 + 321, plans[-1]
    _dense16(launches)


# ---------------------------------------------------------------- keys
def _check_keys(dev, ab, oracle, capfd, hk, kb=None, bpk=10):
    kb = _kb([len(hk)]) if kb is None else kb
    want = _want(oracle, hk, kb, bpk)
    capfd.readouterr()
    _three_builds(dev, ab, kb, dev.from_numpy(hk).cuda(), want, bpk)
    return _lines(capfd)


@pytest.mark.parametrize("dedup", ["1", "0"])
def test_identical_keys(dev, ab, oracle, small, capfd, dedup):
    """10 000 times one key: six hot tiles at most, so a counter reaches up to
    K * C in every chunk; with the repeated-pair table and without it
    (ADL_BLOOM_HASH_DEDUP=0)."""
    small.set("ADL_BLOOM_HASH_DEDUP", dedup)
    hk = np.tile(oracle.splitmix_keys16(0x1DE7, 1), (10_000, 1))
    plans, launches = _check_keys(dev, ab, oracle, capfd, hk)
    assert plans[-1]["chunks"] == 40
    _dense16(launches)


def test_identical_keys_several_chunks_per_workgroup(dev, ab, oracle, small, capfd, G):
    """The same with three chunks per workgroup: the hot counters are cleared
    and filled again from step to step."""
    hk = np.tile(oracle.splitmix_keys16(0x1DE8, 1), (3 * G * CK, 1))
    plans, launches = _check_keys(dev, ab, oracle, capfd, hk)
    assert plans[-1]["chunks"] == 3 * G
    _dense16(launches)


def test_converged_pairs_across_chunks(dev, ab, oracle, small, capfd, G):
    """Keys of bytes >= 0x80 whose two hashes are equal (the pairs the
    repeated-pair table skips), each many times and spread over all the
    chunks of every workgroup; two filters, so the table is cleared between."""
    rng = np.random.default_rng(0x80)
    cand = rng.integers(0x80, 0x100, (40_000, 16), dtype=np.uint8)
    h = oracle.murmur3_batch(cand)
    conv = cand[h[:, 0] == h[:, 1]]
    assert len(conv) >= 200, len(conv)
    n = 2 * G * CK + 999
    hk = conv[rng.integers(0, 200, n)]
    kb = _kb([n // 2, n - n // 2])
    plans, launches = _check_keys(dev, ab, oracle, capfd, hk, kb)
    assert plans[-1]["chunks"] > 2 * G
    _dense16(launches)


@pytest.mark.parametrize("bpk", [0, 44])
def test_bpk_edges(dev, ab, oracle, small, capfd, G, bpk):
    """bpk 0 (one tile, k = 1) and bpk 44 (k = 30): not the k = 6 kernel but
    the generic pass A, through the same plan and pass B."""
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [G * CK + 1], bpk)
    assert launches and all(l[1] == "generic bloom_bin_kernel" for l in launches), launches


def test_one_tile_filters(dev, ab, oracle, small, capfd):
    """T = 1 in the k = 6 kernel: filters of 1 to 9 keys among larger ones."""
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [5, 70_000, 1, 9, 300, 2])
    _dense16(launches)


# ---------------------------------------------------------------- sources and modes
def _varlen(oracle, sizes):
    key = ("var", tuple(sizes))
    if key not in _REF:
        kb = _kb(sizes)
        rng = random.Random(77 + len(sizes))
        keys = [rng.randbytes(rng.randrange(0, 41)) for _ in range(int(kb[-1]))]
        data, offs = oracle.pack(keys)
        pad = np.zeros(((data.size + 15) // 16) * 16 + 32, dtype=np.uint8)
        pad[: data.size] = data
        want = [oracle.keys2block(keys[int(kb[f]):int(kb[f + 1])]) for f in range(len(sizes))]
        _REF[key] = (kb, pad, offs, want)
    return _REF[key]


SHAPES = {"ragged": [2 * 256 * CK + 1], "boundaries": [30_000, 100, 60_000]}


@pytest.mark.parametrize("queues", ["static", "queued"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_src16_queued(dev, ab, oracle, small, capfd, shape, queues):
    """16-byte keys, chunks in the static order and from the work queues
    (ADL_BLOOM_BUILD_QUEUES=3: a workgroup's next chunk may be any filter's)."""
    if queues == "queued":
        small.set("ADL_BLOOM_BUILD_QUEUES", "3")
    plans, launches = _run_fixed(dev, ab, oracle, capfd, SHAPES[shape])
    _dense16(launches, queues)


@pytest.mark.parametrize("queues", ["static", "queued"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_srch(dev, ab, oracle, small, capfd, shape, queues):
    """Variable-length keys (0-40 bytes, k = 6) in a 16-byte-aligned buffer:
    the hashing pass, then pass A over its pairs."""
    if queues == "queued":
        small.set("ADL_BLOOM_BUILD_QUEUES", "3")
    kb, pad, offs, want = _varlen(oracle, SHAPES[shape])
    data = dev.from_numpy(pad).cuda()
    assert data.data_ptr() % 16 == 0
    capfd.readouterr()
    _three_builds(dev, ab, kb, data, want, offsets=dev.from_numpy(offs.view(np.int64)).cuda())
    plans, launches = _lines(capfd)
    assert launches and all(l[0] == queues and l[1] == "bin16 SrcH dense" for l in launches), launches


@pytest.mark.parametrize("queues", ["static", "queued"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_srcp(dev, ab, oracle, small, capfd, shape, queues):
    """A StreamBuilder's finish: pass A over the stream's stored pairs, three
    times into the same workspace and bitmaps."""
    if queues == "queued":
        small.set("ADL_BLOOM_BUILD_QUEUES", "3")
    kb, hk, want = _fixed(oracle, SHAPES[shape])
    sb = ab.StreamBuilder()
    for f in range(len(want)):
        sb.append(hk[int(kb[f]):int(kb[f + 1])])
        sb.cut()
    capfd.readouterr()
    boff, sizes, total = sb._layout(10)
    ws_bytes = sb.workspace_bytes(10)
    out = ab.empty_device(total)
    ws = ab.empty_device(ws_bytes)
    for r in range(3):
        ab._check(ab.lib().adl_bloom_stream_finish_device(sb._h, 10, 0, ctypes.c_void_p(out.data_ptr()),
                                                          boff.ctypes.data, ctypes.c_void_p(ws.data_ptr()), ws_bytes,
                                                          ab._stream(None)), "adl_bloom_stream_finish_device")
        dev.cuda.synchronize()
        got = out.cpu().numpy()
        for f, w in enumerate(want):
            assert np.array_equal(got[int(boff[f]):int(boff[f]) + int(sizes[f])], w), f"finish {r}, filter {f}"
    sb.close()
    plans, launches = _lines(capfd)
    assert launches and all(l[0] == queues and l[1] == "bin16 SrcP dense" for l in launches), launches


def test_claim_layout_unchanged(dev, ab, oracle, knobs, capfd):
    """304 filters of 300 keys (at most 10 tiles each): the plan picks the
    claim layout, whose loop keeps its two counter arrays and its barriers."""
    knobs.set("ADL_BLOOM_DEBUG", "1")
    plans, launches = _run_fixed(dev, ab, oracle, capfd, [300] * 304)
    assert plans[-1]["claim"]
    assert launches and all(l[1] == "bin16 Src16 claim" for l in launches), launches
