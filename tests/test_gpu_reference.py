"""GPU: the device paths against the reference's compiled src/filter_block.cpp.

Every other GPU test compares a kernel with the oracle (oracle/bloom_oracle.c,
oracle/oracle.py), a restatement of the reference written beside the kernels.
This file does not consult the oracle: what a kernel wrote is compared, by
SHA-256 or byte for byte, with tests/golden/filter_block_ref.json, which
tests/golden/make_filter_block_ref.py recorded from the reference's
BloomFilter, FilterBlockWriter and FilterBlockReader compiled unmodified
(oracle/_ref/libref_filter_block.so).  Where that library is on the machine,
test_live_reference_is_the_recorded_one first proves that it still answers what
the JSON holds.  The cases and their inputs are tests/refcases.py; a mistake
shared by the oracle and the kernels (the signedness of j * h2, the clamp of
k, the int conversions around h % m) fails here.

Shapes are the smallest that reach each kernel, and the kernel that ran is
read from the "adl_bloom launch:" line of ADL_BLOOM_DEBUG=1.
"""
import re

import numpy as np
import pytest

import refcases as C

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"adl_bloom launch: pass A (?:queued|static) \((.+?), (?:DT|kernarg)\)")
GENERIC = "generic bloom_bin_kernel"


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
def rec():
    return C.load_json()


def up(dev, a):
    return dev.from_numpy(np.require(a, requirements=["C", "W"])).cuda()


def up_keys(dev, k, shift=0):
    """Packed keys `shift` bytes past a 16-byte boundary (with their 16 spare bytes), and the offsets."""
    buf = dev.zeros(k.data.size + 32, dtype=dev.uint8, device="cuda")
    view = buf[shift:shift + k.data.size]
    view.copy_(dev.from_numpy(k.data))
    assert view.data_ptr() % 16 == shift
    return view, up(dev, k.offs.view(np.int64))


def up_queries(dev, name, s):
    """Queries of a block's case: (n, 16) keys without offsets where the block's keys are 16-byte keys."""
    if C.BLOCKS[name][0] == "split16":
        return up(dev, s.fixed(16)), None
    return up_keys(dev, s)


def test_live_reference_is_the_recorded_one(rec):
    """Where oracle/_ref/libref_filter_block.so is on the machine: the compiled reference answers,
    now, what the JSON the other tests compare with holds (without it the JSON alone decides)."""
    import oracle  # the loader only

    R = oracle.ref_filter_block_lib()
    if R is None:
        return
    ref = C.Ref(R)
    for shape, bpk, n in BUILDS_USED:
        g = rec["builds"][C.build_id(shape, bpk, n)]
        bm = ref.keys2block(bpk, C.members(shape, n))
        assert (len(bm), C.sha(bm)) == (g["bytes"], g["sha256"])
    for name, (shape, bpk, counts) in C.BLOCKS.items():
        g = rec["blocks"][name]
        blk = ref.block(bpk, C.block_keys(name), counts)
        assert (len(blk), C.sha(blk)) == (g["bytes"], g["sha256"])
        assert [[len(b), C.sha(b)] for b in C.split_block(blk)[0]] == g["bitmaps"]
        ids, q = C.block_queries(name)
        assert C.bits_hex(ref.reader_probe(blk, ids, q)) == g["answers"]
    fid, keys = C.binned_queries()
    _, bpk, counts = C.BLOCKS[C.BINNED_BLOCK]
    blk = ref.block(bpk, C.block_keys(C.BINNED_BLOCK), counts)
    qk = C.Keys(keys.reshape(-1), np.arange(C.BINNED_N + 1, dtype=np.uint64) * np.uint64(16))
    assert C.sha(ref.reader_probe(blk, fid, qk).astype(np.uint8).tobytes()) == rec["binned"]["answers_sha256"]
    k3, counts3 = C.base3()
    base = ref.block(C.BASE3_BPK, k3, counts3)
    for name, m in C.mutations(base).items():
        rc, ans = ref.mutation(m)
        assert {"rc": rc, "answers": ans} == rec["mutations"]["cases"][name]


# ---------------------------------------------------------------- adl_bloom_build_device
N16 = (1, 65, 6145, 50_001)
BUILD16 = [(bpk, n) for bpk in C.BPKS for n in N16]
VARLEN = [(n, bpk, staged) for n in (6145, 50_001) for bpk in (10, 44) for staged in (True, False)]
BUILDS_USED = ([("split16", bpk, n) for bpk, n in BUILD16] + list(C.EXTRA_BUILDS) +
               [("varlen", bpk, n) for n, bpk, _ in VARLEN])
# pass A's layout of bloom_bin16_kernel for one filter of n 16-byte keys at k = 6: the claim layout
# for the filters of one tile, the dense one from 6145 keys on (make_plan, bloom_build.hip, keeps the
# claim layout where a tile's share of the region clears its mean run by four standard deviations)
LAYOUT16 = {1: "claim", 65: "claim", 6145: "dense", 50_001: "dense"}


def built(ab, dev, knobs, capfd, keys, offsets, bpk):
    """(bitmap bytes, pass A kernels named by the launch lines) of one adl_bloom_build_device"""
    knobs.set("ADL_BLOOM_DEBUG", "1")
    capfd.readouterr()
    bm = ab.build(keys, offsets, bits_per_key=bpk)
    dev.cuda.current_stream().synchronize()
    got = bm.cpu().numpy().tobytes()
    return got, LAUNCH.findall(capfd.readouterr().err)


@pytest.mark.parametrize("bpk,n", BUILD16)
def test_build_device_16_byte_keys(dev, ab, rec, knobs, capfd, bpk, n):
    """bits_per_key 0..100: k in {1, 2, 3, 6, 7, 11, 13, 20, 29, 30}, the clamp at both ends."""
    g = rec["builds"][C.build_id("split16", bpk, n)]
    k = C.members("split16", n)
    assert k.sha() == rec["inputs"]["split16"]["members"][str(n)]
    got, kern = built(ab, dev, knobs, capfd, up(dev, k.fixed(16)), None, bpk)
    assert len(got) == g["bytes"]
    assert C.sha(got) == g["sha256"]
    if ab.num_probes(bpk) == 6:
        assert kern == ["bin16 Src16 " + LAYOUT16[n]]
    else:
        assert kern == [GENERIC]


@pytest.mark.parametrize("shape,bpk,n", C.EXTRA_BUILDS)
def test_build_device_stride_24(dev, ab, rec, knobs, capfd, shape, bpk, n):
    """Fixed-size keys that are not 16 bytes: KeysStride, the generic pass A at any k."""
    g = rec["builds"][C.build_id(shape, bpk, n)]
    k = C.members(shape, n)
    assert k.sha() == rec["inputs"][shape]["members"][str(n)]
    got, kern = built(ab, dev, knobs, capfd, up(dev, k.fixed(24)), None, bpk)
    assert (len(got), C.sha(got)) == (g["bytes"], g["sha256"])
    assert kern == [GENERIC]


@pytest.mark.parametrize("n,bpk,staged", VARLEN, ids=[f"n{n}-bpk{b}-{'staged' if s else 'unstaged'}"
                                                      for n, b, s in VARLEN])
def test_build_device_var_len_keys(dev, ab, rec, knobs, capfd, n, bpk, staged):
    """Keys of 0 to 69 random bytes (half of them >= 0x80): from a 16-byte aligned buffer the
    hashing pass and bloom_bin16_kernel over its pairs (k = 6) or the staged windows; from an
    unaligned one the generic pass A without staging."""
    g = rec["builds"][C.build_id("varlen", bpk, n)]
    k = C.members("varlen", n)
    assert k.sha() == rec["inputs"]["varlen"]["members"][str(n)]
    dk, do = up_keys(dev, k, 0 if staged else 1)
    got, kern = built(ab, dev, knobs, capfd, dk, do, bpk)
    assert (len(got), C.sha(got)) == (g["bytes"], g["sha256"])
    if bpk == 10 and staged:
        assert kern == ["bin16 SrcH dense"]
    else:
        assert kern == [GENERIC]


@pytest.mark.parametrize("staged", [True, False], ids=["staged", "unstaged"])
def test_build_segmented_var_len_10_filters(dev, ab, rec, knobs, capfd, staged):
    """The 50 001 var-len keys as ten filters through adl_bloom_build_segmented_device_ex: each
    bitmap is the one inside the reference's block of the same ten filters."""
    name = "f10-b10-var50001"
    _, bpk, counts = C.BLOCKS[name]
    k = C.block_keys(name)
    assert k.sha() == rec["blocks"][name]["keys_sha256"]
    kb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    dk, do = up_keys(dev, k, 0 if staged else 1)
    knobs.set("ADL_BLOOM_DEBUG", "1")
    capfd.readouterr()
    out, boff, sizes = ab.build_segmented(dk, kb, do, bits_per_key=bpk)
    assert LAUNCH.findall(capfd.readouterr().err) == ["bin16 SrcH dense" if staged else GENERIC]
    h = out.cpu().numpy()
    got = [h[int(boff[f]):int(boff[f]) + int(sizes[f])] for f in range(len(counts))]
    assert [[b.size, C.sha(b)] for b in got] == rec["blocks"][name]["bitmaps"]


# ---------------------------------------------------------------- whole blocks
def block_inputs(name):
    """(numpy keys, numpy offsets or None, key_begin) in the form the entry points take"""
    shape, bpk, counts = C.BLOCKS[name]
    k = C.block_keys(name)
    kb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    if shape == "split16":
        return k.fixed(16), None, kb
    return k.data, k.offs, kb


_blocks = {}


def device_block(dev, ab, rec, name) -> bytes:
    """The block adl_bloom_filter_block_build_device builds, proven to be the reference's
    (length and SHA-256 of FilterBlockWriter::Final's bytes) -- built once."""
    if name not in _blocks:
        _, bpk, counts = C.BLOCKS[name]
        assert C.block_keys(name).sha() == rec["blocks"][name]["keys_sha256"]
        keys, offs, kb = block_inputs(name)
        if kb[-1] == 0:
            blk = ab.build_filter_block(None, kb, bits_per_key=bpk)
        elif offs is None:
            blk = ab.build_filter_block(up(dev, keys), kb, bits_per_key=bpk)
        else:
            blk = ab.build_filter_block(up(dev, keys), kb, offsets=up(dev, offs.view(np.int64)), bits_per_key=bpk)
        got = blk.cpu().numpy().tobytes()
        g = rec["blocks"][name]
        assert len(got) == g["bytes"] == ab.filter_block_bytes(kb, bpk)
        assert C.sha(got) == g["sha256"]
        _blocks[name] = got
    return _blocks[name]


# pass A of each block's build: both layouts of bloom_bin16_kernel from 16-byte keys and from the
# hashing pass's pairs, the generic kernel for k != 6, and no pass A where there is no key
BLOCK_KERNEL = {
    "f1-b10-var": "bin16 SrcH dense", "f1-b1-s16": GENERIC, "f1-b44-ascii": GENERIC,
    "empties-b1-var": GENERIC, "empties-b10-s16": "bin16 Src16 claim", "empties-b10-var": "bin16 SrcH claim",
    "empties-b44-var": GENERIC, "all-empty-b10": "none", "f70-b10-s16": "bin16 Src16 dense",
    "f70-b44-var": GENERIC, "f10-b10-var50001": "bin16 SrcH dense",
}


@pytest.mark.parametrize("name", list(C.BLOCKS))
def test_filter_block_build_device(dev, ab, rec, knobs, capfd, name):
    """F = 1 and 70, empty filters first, last and adjacent, bits_per_key 1, 10 and 44."""
    knobs.set("ADL_BLOOM_DEBUG", "1")
    capfd.readouterr()
    _blocks.pop(name, None)
    device_block(dev, ab, rec, name)
    assert LAUNCH.findall(capfd.readouterr().err) == [BLOCK_KERNEL[name]]


@pytest.mark.parametrize("name", list(C.BLOCKS))
def test_filter_cache_build(dev, ab, rec, name):
    """FilterCache.build (write-through, host keys): the block it returns for the file is the
    reference's, and so is what it left resident -- the recorded answers for every id 0..F+1."""
    _, bpk, counts = C.BLOCKS[name]
    g = rec["blocks"][name]
    keys, offs, kb = block_inputs(name)
    cache = ab.FilterCache(16 << 20, max_tables=4)
    try:
        blk, ticket = cache.build(keys if kb[-1] else np.zeros((0, 16), np.uint8), kb, offs if kb[-1] else None,
                                  bits_per_key=bpk)
        assert (len(blk), C.sha(blk)) == (g["bytes"], g["sha256"])
        cache.publish(ticket, b"t")
        ids, q = C.block_queries(name)
        want = C.hex_bits(g["answers"], q.n)
        got = np.empty(q.n, np.uint8)
        for f in range(len(counts) + 2):
            a, b = np.searchsorted(ids, [f, f + 1])
            s = q.slice(int(a), int(b))
            got[a:b], unc = cache.probe([b"t"], np.zeros(s.n, np.uint32), s.data, s.offs, filter=f)
            assert unc == 0
        assert np.array_equal(got, want)
    finally:
        cache.close()


# ---------------------------------------------------------------- probes
def block_case(dev, ab, rec, name):
    """(block, offsets F+1, filter ids, queries, the reference's answers)"""
    blk = device_block(dev, ab, rec, name)
    _, off = C.split_block(blk)
    ids, q = C.block_queries(name)
    g = rec["blocks"][name]
    assert C.sha(ids.astype("<i4").tobytes() + bytes.fromhex(q.sha())) == g["queries_sha256"]
    want = C.hex_bits(g["answers"], q.n)
    F = len(off) - 1
    assert set(ids.tolist()) == set(range(F + 2)) and not want[ids >= F].any()
    return blk, off, ids, q, want


@pytest.mark.parametrize("name", list(C.BLOCKS))
def test_probe_device(dev, ab, rec, name):
    """adl_bloom_probe_device, one filter at a time."""
    blk, off, ids, q, want = block_case(dev, ab, rec, name)
    bpk = C.BLOCKS[name][1]
    arena = up(dev, np.frombuffer(blk, dtype=np.uint8))
    for f in range(len(off) - 1):
        a, b = np.searchsorted(ids, [f, f + 1])
        s = q.slice(int(a), int(b))
        dk, do = up_queries(dev, name, s)
        bm = arena[int(off[f]):int(off[f + 1])]
        got = ab.probe(dk, bm, offsets=do, bits_per_key=bpk).cpu().numpy()
        assert np.array_equal(got, want[a:b]), f


@pytest.mark.parametrize("name", list(C.BLOCKS))
def test_probe_multi_and_filter_set(dev, ab, rec, name):
    """adl_bloom_probe_multi_device and adl_bloom_filter_set_probe over the block's bitmaps, ids F
    and F+1 included."""
    blk, off, ids, q, want = block_case(dev, ab, rec, name)
    bpk = C.BLOCKS[name][1]
    arena = np.frombuffer(blk, dtype=np.uint8)
    dk, do = up_queries(dev, name, q)
    got = ab.probe_multi(dk, up(dev, ids), up(dev, arena), up(dev, off.view(np.int64)), offsets=do,
                         bits_per_key=bpk).cpu().numpy()
    assert np.array_equal(got, want)
    fs = ab.FilterSet(arena, off, bits_per_key=bpk)
    try:
        assert np.array_equal(fs.probe(q.data, filter_id=ids.view(np.uint32), offsets=q.offs), want)
        F = len(off) - 1
        for f in (0, F - 1, F, F + 1):  # one filter for the whole batch
            a, b = np.searchsorted(ids, [f, f + 1])
            s = q.slice(int(a), int(b))
            assert np.array_equal(fs.probe(s.data, filter=f, offsets=s.offs), want[a:b]), f
    finally:
        fs.close()


@pytest.mark.parametrize("name", list(C.BLOCKS))
def test_probe_fanout(dev, ab, rec, name):
    """adl_bloom_probe_fanout_device: every distinct query key once, with the list of all the
    filter ids it was recorded for (the non-members of ids 2j and 2j+1 are the same keys)."""
    blk, off, ids, q, want = block_case(dev, ab, rec, name)
    bpk = C.BLOCKS[name][1]
    first, lists = {}, []
    for i in range(q.n):
        key = q.key(i)
        if key not in first:
            first[key] = len(lists)
            lists.append([])
        lists[first[key]].append(i)
    assert max(len(p) for p in lists) >= 2
    order = np.array([i for p in lists for i in p])
    uniq = C.from_list(list(first))
    pb = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32)
    dk, do = up_keys(dev, uniq)
    got = ab.probe_fanout(dk, up(dev, pb), up(dev, ids[order]), up(dev, np.frombuffer(blk, dtype=np.uint8)),
                          up(dev, off.view(np.int64)), offsets=do, bits_per_key=bpk).cpu().numpy()
    assert np.array_equal(got, want[order])


@pytest.mark.parametrize("server", ["1", "0"])
@pytest.mark.parametrize("name", ["f1-b10-var", "empties-b1-var", "empties-b10-var", "empties-b44-var",
                                  "f70-b10-s16", "f70-b44-var"])
def test_filter_cache_probe(dev, ab, rec, knobs, name, server):
    """adl_bloom_filter_cache_put of the block, then multi-gets of 1, 8 and 1000 queries per filter
    id (up to 8 go to the resident probe server, or with ADL_BLOOM_PROBE_SERVER=0 to a launch), and the
    same answers from adl_bloom_filter_cache_probe_fanout over two copies of the block."""
    blk, off, ids, q, want = block_case(dev, ab, rec, name)
    knobs.set("ADL_BLOOM_PROBE_SERVER", server)
    F = len(off) - 1
    cache = ab.FilterCache(16 << 20, max_tables=4)
    try:
        cache.put(b"oid", blk)
        cache.put(b"oid2", blk)
        for f in list(range(min(F, 12))) + [F - 1, F, F + 1]:
            a, b = np.searchsorted(ids, [f, f + 1])
            assert b - a >= 8
            for batch in (1, 8, 1000):
                idx = (np.arange(batch) % (b - a)) + a
                s = C.from_list([q.key(int(i)) for i in idx])
                got, unc = cache.probe([b"oid"], np.zeros(batch, np.uint32), s.data, s.offs, filter=f)
                assert unc == 0
                assert np.array_equal(got, want[idx]), (f, batch)
                if batch > 1:
                    # adl_bloom_filter_cache_probe_fanout: half as many keys, each against both copies
                    # of the block (8 pairs go the way of the multi-get above, 1000 to the fan-out kernel)
                    h = C.from_list([q.key(int(i)) for i in idx[:batch // 2]])
                    got, unc = cache.probe_fanout([b"oid", b"oid2"], np.arange(0, batch + 1, 2, dtype=np.uint32),
                                                  np.tile(np.array([0, 1], np.uint32), batch // 2), h.data, h.offs,
                                                  filter=f)
                    assert unc == 0
                    assert np.array_equal(got, np.repeat(want[idx[:batch // 2]], 2)), (f, batch, "fanout")
    finally:
        cache.close()


def test_probe_batch_binned(dev, ab, rec):
    """adl_bloom_probe_batch_device's tile-binned pipeline (16-byte keys, n >= 2^20): 2^20 + 777
    queries over the 70-filter block at bits_per_key 10; the answers' SHA-256 is the reference's."""
    g = rec["binned"]
    blk = device_block(dev, ab, rec, g["block"])
    _, off = C.split_block(blk)
    fid, keys = C.binned_queries()
    assert g["n"] == len(fid) == C.BINNED_N >= 1 << 20
    assert C.sha(fid.astype("<i4").tobytes() + keys.tobytes()) == g["queries_sha256"]
    got = ab.probe_batch(up(dev, keys), up(dev, fid), up(dev, np.frombuffer(blk, dtype=np.uint8)),
                         up(dev, off.view(np.int64)), bits_per_key=C.BLOCKS[g["block"]][1]).cpu().numpy()
    assert int(got.sum()) == g["ones"]
    assert C.sha(got.tobytes()) == g["answers_sha256"]


# ---------------------------------------------------------------- the cache's trailer parse
# Trailer mutations adl_bloom_filter_cache_put rejects although the reference's Init accepts them,
# with the reason adlsm-tree_amd/csrc/filter_block_format.hpp gives.  The same list as the oracle's
# (tests/test_oracle_reference_cpu.py).
REJECTED_THOUGH_REFERENCE_ACCEPTS = {
    "F=-1": "a negative filter count: nf < 0 is refused (the reference answers 0 for every id)",
    "F=1000": "the offsets array must lie inside the block, before the count field; the reference's "
              "IsKeyExists reads its entries beyond the block",
    "off_1>off_2": "offsets out of order: the reference forms a bitmap of negative length and reads outside it",
    "off_2>offsets_start": "an offset beyond offsets_start: the last filter's range would have negative length",
}
# Accepted by both, but one filter id is an empty range: the reference computes h % 0
# (src/filter_block.cpp:56), the probe answers 0 (adlsm-tree_amd/csrc/probe_device.hpp).
EMPTY_RANGE_ANSWERS_0 = {
    "F=4": "filter 3's offset is the offsets_start field itself, so filter 3 is [offsets_start, offsets_start)",
}
MUTATION_NAMES = sorted(C.mutations(bytes(33) + b"".join(int(v).to_bytes(4, "little") for v in (0, 11, 22, 33, 3)) +
                                    b"bf:" + (10).to_bytes(4, "little") + (7).to_bytes(4, "little")))


@pytest.fixture(scope="module")
def base3(dev, ab, rec):
    """The well-formed 3-filter block, built on the device and proven to be the reference's."""
    k, counts = C.base3()
    kb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    blk = ab.build_filter_block(up(dev, k.data), kb, offsets=up(dev, k.offs.view(np.int64)),
                                bits_per_key=C.BASE3_BPK).cpu().numpy().tobytes()
    g = rec["mutations"]["base"]
    assert (len(blk), C.sha(blk)) == (g["bytes"], g["sha256"])
    return C.mutations(blk)


@pytest.mark.parametrize("name", MUTATION_NAMES)
def test_cache_put_trailer_mutation(ab, rec, base3, name):
    """adl_bloom_filter_cache_put's status for each mutated trailer, and for the accepted ones
    the cache's answers for ids 0..5 and 999..1001, under the reader rule (refcases.check_reader_rule)."""
    assert set(rec["mutations"]["cases"]) == set(MUTATION_NAMES)
    blk = base3[name]
    cache = ab.FilterCache(4 << 20, max_tables=4)
    try:
        rc = cache.put_status(b"m", blk)
        keys = C.from_list(list(C.MUT_KEYS))
        answers = {}

        def exists(i, key):
            if i not in answers:
                got, unc = cache.probe([b"m"], np.zeros(keys.n, np.uint32), keys.data, keys.offs, filter=i)
                assert unc == 0
                answers[i] = dict(zip(C.MUT_KEYS, got.tolist()))
            return answers[i][key]

        C.check_reader_rule(name, rec["mutations"]["cases"][name], rc, exists, REJECTED_THOUGH_REFERENCE_ACCEPTS,
                            EMPTY_RANGE_ANSWERS_0)
        assert (b"m" in cache) == (rc == 0)
    finally:
        cache.close()
