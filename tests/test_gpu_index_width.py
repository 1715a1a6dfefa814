"""GPU: indices, offsets and counts past 32 bits.

include/adl_bloom.h takes uint64_t key counts, key offsets, key_begin,
bitmap_off and d_begin / d_end, and the rest of the suite stops short of 2^32
in every one of them.  Each case here moves one of them across a boundary and
compares with the oracle (oracle.keys2block / probe / probe_multi: the
reference's BloomFilter::Keys2Block and IsKeyExists, src/filter_block.cpp:9-62)
with `==`, on the small host copies of the keys and bitmaps the case uses:

  1  builds whose keys lie past byte 2^32 of the key buffer (16-byte keys, a
     24-byte stride, variable-length keys with offsets[0] = 2^32 - 150 000)
  2  probe, verify and murmur3 over such keys; 2^28 + 4096 generated 16-byte
     keys (the generator's own stores, and a probe of all of them)
  3  the tile-binned probe at n = 2^28 + 2^20 + 777: its entry array, hash
     array and key buffer pass 4 GiB
  4  bitmaps read and written at arena offsets past 2^32
  5  filters of 2^31 - 8 bits (the largest) and of 2^31 bits (answers 0)
  6  the launch-group split of a segmented build (a second group)
  7  a filter cache whose arena bases pass 4 GiB

`big` is one uninitialised device buffer of 2^32 + 2^26 bytes: key buffer,
arena or output of cases 1-4, which write and read only their own windows.
Nothing of 4 GiB exists on the host.  Where a case is about one kernel, it
asserts the `adl_bloom launch:` line (ADL_BLOOM_DEBUG=1) as
test_gpu_build_queues.py does.  Figures measured on an MI355X are in the
docstrings of the cases they belong to.
"""
import ctypes
import gc
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B32 = 1 << 32
BIG_BYTES = B32 + (1 << 26)
LAUNCH = re.compile(r"adl_bloom launch: pass A (queued|static) \((.+?), (DT|kernarg)\), "
                    r"pass B (queued|static) \((\d) per CU, (DT|kernarg)\)")
GENERIC = "generic bloom_bin_kernel"
ADL_ERR_WORKSPACE = -5
NONE64 = (1 << 64) - 1


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


@pytest.fixture(scope="module", autouse=True)
def peak(dev):
    """Prints the file's peak of torch's device allocations (the filter cache's
    arena of case 7, 6 GiB, is the library's own hipMalloc and not in it)."""
    dev.cuda.reset_peak_memory_stats()
    yield
    print(f"\ntest_gpu_index_width: peak device memory {dev.cuda.max_memory_allocated()} bytes")


@pytest.fixture(scope="module")
def big(dev, peak):
    t = dev.empty(BIG_BYTES, dtype=dev.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    yield t
    t.untyped_storage().resize_(0)  # (the fixture's cached value still refers to the tensor)
    dev.cuda.empty_cache()


@pytest.fixture(autouse=True)
def release(dev):
    """Workspaces of 10 GB go back to the device after the case that used them."""
    yield
    gc.collect()
    dev.cuda.synchronize()
    dev.cuda.empty_cache()


# ---------------------------------------------------------------- helpers
def _d(dev, a):
    """Host array -> device tensor (uint64 / uint32 travel as int64 / int32)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return dev.from_numpy(a).cuda()


def _put(dev, buf, at, a):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf[at:at + a.size] = dev.from_numpy(a).cuda()


def _get(buf, at, n):
    return buf[at:at + n].cpu().numpy()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(dev):
    return ctypes.c_void_p(dev.cuda.current_stream().cuda_stream)


def _kb(sizes, first=0):
    return (np.concatenate([[0], np.cumsum(sizes)]) + first).astype(np.uint64)


def _debug(knobs, capfd):
    knobs.set("ADL_BLOOM_DEBUG", "1")
    capfd.readouterr()


def _launches(capfd):
    return [m.groups() for m in LAUNCH.finditer(capfd.readouterr().err)]


def _assert_launch(line, kernel, dt):
    """Pass A's kernel and where the descriptors came from (the order of the
    items and pass B's occupancy are the plan's business, not these cases')."""
    assert line[1].startswith(kernel), line
    assert line[2] == line[5] == ("DT" if dt else "kernarg"), line


def _check_filters(out, boff, want):
    """Every filter's bitmap equals the oracle's and its pad bytes up to the
    16-byte allocation are 0."""
    out = out.cpu().numpy()
    for f, w in enumerate(want):
        alloc = (w.size + 15) // 16 * 16
        got = out[int(boff[f]):int(boff[f]) + alloc]
        assert np.array_equal(got[:w.size], w), f"filter {f} of {len(want)}"
        assert not got[w.size:].any(), f"pad of filter {f}"


def _ranges(dev, ab, keys, offs, n, stride, fid, nf, bitmaps, begin, end, bpk):
    out = dev.empty(n, dtype=dev.uint8, device="cuda")
    rc = ab.lib().adl_bloom_probe_ranges_device(_p(keys), _p(offs), n, stride, _p(fid), nf, _p(bitmaps), _p(begin),
                                                _p(end), bpk, _p(out), _stream(dev))
    assert rc == 0
    return out.cpu().numpy()


def _fanout(dev, ab, keys, offs, n, stride, lists, nf, bitmaps, begin, end, bpk):
    """lists[i]: the filter ids key i probes.  Returns one answer per pair."""
    pb = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    pf = np.concatenate(lists).astype(np.uint32)
    out = dev.empty(pf.size, dtype=dev.uint8, device="cuda")
    d_pb, d_pf = _d(dev, pb), _d(dev, pf)
    rc = ab.lib().adl_bloom_probe_fanout_device(_p(keys), _p(offs), n, stride, _p(d_pb), _p(d_pf), pf.size, nf,
                                                _p(bitmaps), _p(begin), _p(end), bpk, _p(out), _stream(dev))
    assert rc == 0
    return out.cpu().numpy(), pf


def _verify(dev, ab, keys, offs, n, stride, key_begin, nf, bitmaps, begin, end, bpk):
    res = dev.empty(2, dtype=dev.int64, device="cuda")
    d_kb = _d(dev, np.asarray(key_begin, np.uint64))
    rc = ab.lib().adl_bloom_verify_device(_p(keys), _p(offs), n, stride, _p(d_kb), nf, _p(bitmaps), _p(begin), _p(end),
                                          bpk, _p(res), _stream(dev))
    assert rc == 0
    r = res.cpu().numpy().view(np.uint64)
    return int(r[0]), int(r[1])


def _segmented(dev, ab, keys, stride, kb, bpk, out, boff, ws, ws_bytes, flags=0):
    kb = np.ascontiguousarray(kb, dtype=np.uint64)
    boff = np.ascontiguousarray(boff, dtype=np.uint64)
    rc = ab.lib().adl_bloom_build_segmented_device_ex(_p(keys), None, stride, kb.ctypes.data, len(kb) - 1, bpk,
                                                      _p(out), boff.ctypes.data, flags, _p(ws), ws_bytes, _stream(dev))
    dev.cuda.synchronize()
    return rc


_REF = {}  # inputs and the oracle's answers, computed once


# ================================================================ 1. builds from keys past byte 2^32
S3 = [20000, 0, 5000]                                             # <= 8 filters: descriptors in the kernarg
S12 = [20000, 0, 5000, 1, 300, 4097, 0, 777, 2500, 13, 1000, 64]  # > 8: the device FilterTable
CROSS = 7001  # key CROSS of filter 0 is the first past byte 2^32 (no multiple of 4: never a chunk's first key)


def _fixed(oracle, sizes, bpk, stride, dups):
    key = ("fixed", tuple(sizes), bpk, stride, dups)
    if key not in _REF:
        kb = _kb(sizes)
        n = int(kb[-1])
        if stride == 16:
            hk = oracle.splitmix_keys16(0x1D00 + len(sizes), n)
        else:
            hk = np.random.default_rng(stride).integers(0, 256, (n, stride), dtype=np.uint8)
        if dups:
            # runs of 1-5 equal keys; keys CROSS-1 .. CROSS+1 are one run, which lies across byte 2^32
            src = np.repeat(np.arange(n), np.random.default_rng(5).integers(1, 6, n))[:n]
            hk = hk[src]
            hk[CROSS - 1:CROSS + 2] = hk[CROSS - 1]
        want = [oracle.keys2block(hk[int(kb[f]):int(kb[f + 1])], bits_per_key=bpk) for f in range(len(sizes))]
        _REF[key] = (kb, hk, want)
    return _REF[key]


@pytest.mark.parametrize("sizes,bpk,stride,dups,kernel", [
    (S3, 10, 16, False, "bin16 Src16"),
    (S12, 10, 16, False, "bin16 Src16"),
    (S3, 20, 16, False, GENERIC),
    (S3, 10, 24, False, GENERIC),
    (S3, 10, 16, True, GENERIC),
], ids=["kernarg", "table", "bpk20", "stride24", "adjacent-duplicates"])
def test_build_fixed_keys_past_4gib(dev, ab, oracle, knobs, capfd, big, sizes, bpk, stride, dups, kernel):
    """key_begin[0] = 2^28 - 7001 (stride 16) or 2^32 / 24 - 7001 (stride 24):
    filter 0's 20 000 keys begin below byte 2^32 of the key buffer and end
    above it, inside a chunk; every other filter lies above.  bin16 (k = 6,
    16-byte keys), the generic kernel with a runtime k over Keys16 (bpk 20), a
    24-byte stride (the key at 2^32 - 16 itself lies across the boundary), and
    ADL_BLOOM_SKIP_ADJACENT_DUPLICATES, whose same_as_prev compares the key at
    byte 2^32 with the one below it."""
    kb, hk, want = _fixed(oracle, sizes, bpk, stride, dups)
    k0 = B32 // stride - CROSS
    assert k0 * stride < B32 < (k0 + sizes[0]) * stride and (k0 + int(kb[-1])) * stride <= BIG_BYTES
    assert (k0 + CROSS) * stride <= B32 < (k0 + CROSS + 1) * stride
    _put(dev, big, k0 * stride, hk)
    keys = big[:BIG_BYTES // stride * stride].view(-1, stride)
    _debug(knobs, capfd)
    out, boff, _ = ab.build_segmented(keys, kb + np.uint64(k0), bits_per_key=bpk,
                                      flags=ab.SKIP_ADJACENT_DUPLICATES if dups else 0)
    _check_filters(out, boff, want)
    lines = _launches(capfd)
    assert len(lines) == 1
    _assert_launch(lines[0], kernel, len(sizes) > 8)


VOFF = B32 - 150_000      # offsets[0] of the variable-length key sets
VSIZES = [17000, 3000, 10000]


def _varkeys(oracle):
    """30 000 keys of 0-300 bytes and six of 5 000: (keys, packed bytes, offsets from 0)."""
    if "var" not in _REF:
        rng = random.Random(32)
        keys = [rng.randbytes(rng.randrange(0, 301)) for _ in range(sum(VSIZES))]
        for i in (3, 998, 16999, 17000, 20001, 29999):
            keys[i] = rng.randbytes(5000)
        data, offs = oracle.pack(keys)
        assert 150_000 < int(offs[-1]) < (1 << 26) - 64 and 150_000 not in offs  # a key lies across byte 2^32
        _REF["var"] = (keys, data, offs)
    return _REF["var"]


def _var_want(oracle, bpk, first):
    key = ("var-want", bpk, first)
    if key not in _REF:
        keys = _varkeys(oracle)[0]
        kb = _kb(VSIZES)
        kb[0] = first
        _REF[key] = (kb, [oracle.keys2block(keys[int(kb[f]):int(kb[f + 1])], bits_per_key=bpk) for f in range(3)])
    return _REF[key]


@pytest.mark.parametrize("shift,bpk,first,kernel", [
    (0, 10, 0, "bin16 SrcH"),
    (0, 20, 0, GENERIC),
    (1, 10, 0, GENERIC),
    (0, 10, 5, "bin16 SrcH"),
], ids=["aligned-bpk10", "aligned-bpk20", "base+1", "key_begin5"])
def test_build_varlen_keys_past_4gib(dev, ab, oracle, knobs, capfd, big, shift, bpk, first, kernel):
    """offsets[0] = 2^32 - 150 000, so all but the first thousand keys lie
    past byte 2^32: the hashing pass and bin16 over its pairs (aligned base,
    k = 6), the generic kernel staging keys in LDS (bpk 20), the same unstaged
    (base + 1), and key_begin[0] = 5 (offsets[0] belongs to no filter)."""
    keys, data, offs = _varkeys(oracle)
    kb, want = _var_want(oracle, bpk, first)
    base = big[shift:]
    assert base.data_ptr() % 16 == shift
    _put(dev, base, VOFF, data)
    d_offs = _d(dev, offs + np.uint64(VOFF))
    _debug(knobs, capfd)
    out, boff, _ = ab.build_segmented(base, kb, offsets=d_offs, bits_per_key=bpk)
    _check_filters(out, boff, want)
    lines = _launches(capfd)
    assert len(lines) == 1
    _assert_launch(lines[0], kernel, False)


# ================================================================ 2. probe, verify, hash keys past byte 2^32
def test_probe_verify_hash_varlen_keys_past_4gib(dev, ab, oracle, big):
    """The key set of case 1 as queries: key i probes filter (i // 2) % 3 and is
    one of its keys when i is even.  probe, probe_multi, probe_ranges, fan-out
    (2-3 filters per key, one id past the last filter), verify and murmur3."""
    keys, data, offs = _varkeys(oracle)
    n = len(keys)
    idx = np.arange(n)
    fid = ((idx // 2) % 3).astype(np.uint32)
    bms = [oracle.keys2block([keys[i] for i in range(0, n, 2) if fid[i] == f]) for f in range(3)]
    bms.append(oracle.keys2block(keys[0::2]))  # one filter holding every even key: probe_device
    off = _kb([b.size for b in bms])
    arena = np.concatenate(bms + [np.zeros(16, np.uint8)])
    hit = np.stack([oracle.probe(data, b, offsets=offs) for b in bms])  # hit[f, i]: key i in filter f
    assert hit[3, 0::2].all() and 0 < hit[3, 1::2].sum() < n // 4

    _put(dev, big, VOFF, data)
    d_offs = _d(dev, offs + np.uint64(VOFF))
    d_arena, d_off, d_fid = _d(dev, arena), _d(dev, off), _d(dev, fid)
    o3 = int(off[3])
    got = ab.probe(big, d_arena[o3:], nbytes=bms[3].size, offsets=d_offs).cpu().numpy()
    assert np.array_equal(got, hit[3])
    want = hit[fid, idx]
    assert want[0::2].all()
    got = ab.probe_multi(big, d_fid, d_arena, d_off[:4], offsets=d_offs).cpu().numpy()
    assert np.array_equal(got, want)
    got = _ranges(dev, ab, big, d_offs, n, 0, d_fid, 3, d_arena, d_off[:3], d_off[1:4].contiguous(), 10)
    assert np.array_equal(got, want)
    lists = [[int(fid[i]), (int(fid[i]) + 1) % 3] + ([3] if i % 3 == 0 else []) for i in range(n)]
    got, pf = _fanout(dev, ab, big, d_offs, n, 0, lists, 3, d_arena, d_off[:4], None, 10)
    owner = np.repeat(idx, [len(x) for x in lists])
    assert np.array_equal(got, np.where(pf < 3, hit[np.minimum(pf, 2), owner], 0))
    # verify: keys [kb[f], kb[f+1]) against filter f -- most are not in it, and each of those counts
    kb = _kb(VSIZES)
    owner = np.repeat(np.arange(3), VSIZES)
    miss = np.nonzero(hit[owner, idx] == 0)[0]
    assert 0 < miss.size < n
    assert _verify(dev, ab, big, d_offs, n, 0, kb, 3, d_arena, d_off[:4], None, 10) == (miss.size, int(miss[0]))
    got = ab.murmur3_batch(big, offsets=d_offs).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, oracle.murmur3_batch(data, offs))


def test_synth_and_probe_fixed_keys_past_4gib(dev, ab, oracle, big):
    """2^28 + 4096 generated 16-byte keys: the keys around byte 2^32 are the
    generator's (its own 64-bit stores), and one probe of all of them against
    a filter of the keys [2^28 - 2000, 2^28 + 18 000) of the same stream
    answers as the oracle at the head and around 2^28 (the tail)."""
    seed, n = 0x51D, (1 << 28) + 4096
    w = (1 << 28) - 4096
    assert ab.lib().adl_synth_keys16_device(big.data_ptr(), seed, 0, n, _stream(dev)) == 0
    head, tail = oracle.splitmix_keys16(seed, 4096), oracle.splitmix_keys16(seed, 8192, skip=w)
    assert np.array_equal(_get(big, 0, 4096 * 16).reshape(-1, 16), head)
    assert np.array_equal(_get(big, w * 16, 8192 * 16).reshape(-1, 16), tail)
    bm = oracle.keys2block(oracle.splitmix_keys16(seed, 20000, skip=(1 << 28) - 2000))
    got = ab.probe(big[:n * 16].view(-1, 16), _d(dev, bm))
    assert got.numel() == n
    assert np.array_equal(got[:4096].cpu().numpy(), oracle.probe(head, bm))
    g = got[w:].cpu().numpy()
    assert np.array_equal(g, oracle.probe(tail, bm))
    assert g[4096 - 2000:].all() and not g[:4096 - 2000].all()


# ================================================================ 3. the binned probe past n = 2^28
def _arena(oracle, sizes, bpk=10, seed0=0x5EED):
    """As tests/test_gpu_probe_batch.py builds it."""
    bms = [oracle.keys2block(oracle.splitmix_keys16(seed0 + t, n), bits_per_key=bpk) if n else
           np.zeros(0, np.uint8) for t, n in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum([b.size for b in bms])]).astype(np.uint64)
    arena = np.concatenate(bms + [np.zeros(16, np.uint8)])
    return arena, off


def test_probe_batch_past_2_28_queries(dev, ab, oracle, big):
    """n = 2^28 + 2^20 + 777 queries over 64 tables of 40 000 keys: the key
    buffer (n * 16 bytes) and the entry array (chunks * k * C * 4 = 6.5 GB, at
    workspace offset 2.7 GB) lie across 4 GiB; the hash array (n * 8 = 2.2 GB)
    does not reach it by itself.  probe_batch
    equals probe_multi over all n, but both share the hash, so three windows
    of 4096 (head, around 2^28, tail) and every 1347th query (200 000 of them,
    gathered on the device) are compared with oracle.probe_multi over queries
    the oracle's generator made again (q0 = the query's index), and every query
    flagged as a member answers 1.

    On an MI355X adl_bloom_probe_batch_workspace_bytes gave 9 995 724 800 bytes,
    6.5 GB of them the entries; the case took 0.6 s, a third of it the
    oracle's 200 000 single-query calls."""
    T, per, n = 64, 40_000, (1 << 28) + (1 << 20) + 777
    assert n * 16 <= BIG_BYTES
    wsb = ab.lib().adl_bloom_probe_batch_workspace_bytes(n, T, 10, 16)
    print(f"\ncase 3: probe batch workspace {wsb} bytes")
    assert wsb > B32  # the binned pipeline's plan, not the direct kernel's 256 bytes
    arena, off = _arena(oracle, [per] * T)
    d_arena, d_off = _d(dev, arena), _d(dev, off)
    keys = big[:n * 16].view(-1, 16)
    fid = dev.empty(n, dtype=dev.int32, device="cuda")
    member = dev.empty(n, dtype=dev.uint8, device="cuda")
    seed = 0xFEED
    assert ab.lib().adl_synth_probe_queries_device(_p(keys), _p(fid), _p(member), seed, 0, n, T, 0x5EED, per,
                                                   _stream(dev)) == 0
    got = ab.probe_batch(keys, fid, d_arena, d_off)
    direct = ab.probe_multi(keys, fid, d_arena, d_off)
    assert got.numel() == n and dev.equal(got, direct)
    assert bool(got[member.bool()].all())
    assert int(member.sum(dtype=dev.int64)) > n // 3

    def window(q0, cnt):
        k, f, m = oracle.synth_probe_queries(cnt, seed=seed, q0=q0, num_tables=T, keys_per_table=per)
        assert np.array_equal(keys[q0:q0 + cnt].cpu().numpy(), k)  # the generator's own stores past 4 GiB
        assert np.array_equal(fid[q0:q0 + cnt].cpu().numpy().view(np.uint32), f)
        assert np.array_equal(member[q0:q0 + cnt].cpu().numpy(), m)
        assert np.array_equal(got[q0:q0 + cnt].cpu().numpy(), oracle.probe_multi(k, f, arena, off)), q0

    for q0 in (0, (1 << 28) - 2048, n - 4096):
        window(q0, 4096)
    ns = 200_000
    idx = np.arange(ns, dtype=np.int64) * (n // ns) + 5
    assert (n // ns) % 2 == 1 and idx[-1] < n
    k, f = np.empty((ns, 16), np.uint8), np.empty(ns, np.uint32)
    m = np.empty(ns, np.uint8)
    gen, kp, fp, mp = oracle.lib().oracle_synth_probe_queries, k.ctypes.data, f.ctypes.data, m.ctypes.data
    for j, q in enumerate(idx.tolist()):  # (one query per call: the generator makes runs, not strides)
        gen(seed, q, 1, T, 0x5EED, per, kp + 16 * j, fp + 4 * j, mp + j)
    sample = dev.from_numpy(idx).cuda()
    assert np.array_equal(keys.index_select(0, sample).cpu().numpy(), k)
    assert np.array_equal(fid.index_select(0, sample).cpu().numpy().view(np.uint32), f)
    assert np.array_equal(got.index_select(0, sample).cpu().numpy(), oracle.probe_multi(k, f, arena, off))


# ================================================================ 4. bitmaps at offsets past 2^32
def _four(oracle):
    if "four" not in _REF:
        sizes = [5, 30_000, 70_000, 200_000]
        members = [oracle.splitmix_keys16(900 + t, s) for t, s in enumerate(sizes)]
        bms = [oracle.keys2block(k) for k in members]
        rng = np.random.default_rng(3)
        n = (1 << 20) + 99
        fid = rng.integers(0, 5, n).astype(np.uint32)  # 4: past the last filter
        keys = oracle.splitmix_keys16(11, n)
        ins = rng.random(n) < 0.5
        for t, s in enumerate(sizes):
            sel = np.nonzero(ins & (fid == t))[0]
            keys[sel] = members[t][rng.integers(0, s, sel.size)]
        want = np.zeros(n, np.uint8)
        for t in range(4):
            want[fid == t] = oracle.probe(keys[fid == t], bms[t])
        assert want[ins & (fid < 4)].all() and 0 < want[~ins].sum() < (~ins).sum() // 2
        nf = 50_000  # the fan-out's keys: the first nf queries, each against 2-3 filters
        hit = np.stack([oracle.probe(keys[:nf], b) for b in bms] + [np.zeros(nf, np.uint8)])
        vkeys = np.concatenate(members)  # verify: every filter's own keys, then each against the next filter
        vmiss = np.concatenate([oracle.probe(members[t], bms[(t + 1) % 4]) == 0 for t in range(4)])
        _REF["four"] = (sizes, bms, keys, fid, want, hit, vkeys, vmiss)
    return _REF["four"]


@pytest.mark.parametrize("layout", ["ranges", "contiguous"])
def test_probe_bitmaps_past_4gib(dev, ab, oracle, big, layout):
    """Four bitmaps in `big`.  ranges: filter 1 begins at 2^32 - 1000 and lies
    across the boundary, the others above it in another order with gaps of 333
    bytes (begin / end arrays: probe_ranges, fan-out and verify with d_end,
    probe_batch with d_bitmap_end).  contiguous: back to back from 2^32 - 1000
    (one offset array: probe_multi, fan-out and verify without d_end,
    probe_batch without).  probe_batch has 2^20 + 99 queries: the binned path."""
    sizes, bms, keys, fid, want, hit, vkeys, vmiss = _four(oracle)
    n = keys.shape[0]
    if layout == "ranges":
        begin, end, o = [0] * 4, [0] * 4, B32 - 1000
        for t in (1, 3, 0, 2):
            begin[t], end[t] = o, o + bms[t].size
            o += bms[t].size + 333
        begin, end = np.array(begin, np.uint64), np.array(end, np.uint64)
    else:
        begin = _kb([b.size for b in bms], B32 - 1000)
        end = begin[1:]
    assert begin[1] < B32 < end[1] if layout == "ranges" else begin[1] < B32 < begin[2]
    for t in range(4):
        _put(dev, big, int(begin[t]), bms[t])
    d_keys, d_fid, d_begin = _d(dev, keys), _d(dev, fid), _d(dev, begin)
    d_end = _d(dev, end) if layout == "ranges" else None
    if layout == "ranges":
        got = _ranges(dev, ab, d_keys, None, n, 16, d_fid, 4, big, d_begin, d_end, 10)
    else:
        got = ab.probe_multi(d_keys, d_fid, big, d_begin).cpu().numpy()
    assert np.array_equal(got, want)
    assert ab.lib().adl_bloom_probe_batch_workspace_bytes(n, 4, 10, 16) > 256  # the binned pipeline's plan
    got = ab.probe_batch(d_keys, d_fid, big, d_begin, bitmap_end=d_end).cpu().numpy()
    assert np.array_equal(got, want)
    nf = hit.shape[1]
    lists = [[int(fid[i]), (int(fid[i]) + 1) % 5] + ([(int(fid[i]) + 2) % 5] if i % 2 else []) for i in range(nf)]
    got, pf = _fanout(dev, ab, d_keys, None, nf, 16, lists, 4, big, d_begin, d_end, 10)
    assert np.array_equal(got, hit[pf, np.repeat(np.arange(nf), [len(x) for x in lists])])
    d_vkeys, kb = _d(dev, vkeys), _kb(sizes)
    assert _verify(dev, ab, d_vkeys, None, vkeys.shape[0], 16, kb, 4, big, d_begin, d_end, 10) == (0, NONE64)
    if layout == "ranges":  # filter f's keys against filter f + 1: the oracle's misses, each counted
        miss = np.nonzero(vmiss)[0]
        assert miss.size > 100_000
        r_begin, r_end = _d(dev, np.roll(begin, -1)), _d(dev, np.roll(end, -1))
        assert _verify(dev, ab, d_vkeys, None, vkeys.shape[0], 16, kb, 4, big, r_begin, r_end, 10) == \
            (miss.size, int(miss[0]))


def test_build_bitmaps_past_4gib(dev, ab, oracle, knobs, capfd, big):
    """adl_bloom_build_segmented_device_ex with d_bitmaps = big: the 300 000-key
    filter (several tiles) is written across byte 2^32, the
    others above it.  Each target range, 4096 bytes on either side and the same
    ranges 2^32 lower (where a truncated offset would land) hold 0xAB before
    the build; afterwards the bitmaps are the oracle's, the pad bytes 0 and the
    rest still 0xAB."""
    sizes = [300_000, 5, 0, 20_000]
    kb = _kb(sizes)
    hk = oracle.splitmix_keys16(0xB17, int(kb[-1]))
    want = [oracle.keys2block(hk[int(kb[f]):int(kb[f + 1])]) for f in range(4)]
    alloc = [ab.bitmap_alloc_bytes(s, 10) for s in sizes]
    boff = np.array([B32 - 1_000_000, B32 + (4 << 20) + 48, B32 + (5 << 20) + 112, B32 + (6 << 20) + 176], np.uint64)
    assert boff[0] < B32 < boff[0] + np.uint64(alloc[0]) and not (boff % 16).any()
    G = 4096
    spans = []
    for f in range(4):
        lo, hi = int(boff[f]) - G, int(boff[f]) + alloc[f] + G
        spans.append((lo, hi))
        big[lo:hi] = 0xAB
        big[max(0, lo - B32):hi - B32] = 0xAB
    d_keys = _d(dev, hk)
    wsb = ab.workspace_bytes(sizes, 10)
    ws = ab.empty_device(wsb)
    _debug(knobs, capfd)
    assert _segmented(dev, ab, d_keys, 16, kb, 10, big, boff, ws, wsb) == 0
    lines = _launches(capfd)
    assert len(lines) == 1
    _assert_launch(lines[0], "bin16 Src16", False)
    for f, (lo, hi) in enumerate(spans):
        got = _get(big, lo, hi - lo)
        assert (got[:G] == 0xAB).all() and (got[-G:] == 0xAB).all(), f"guard of filter {f}"
        body = got[G:-G]
        assert np.array_equal(body[:want[f].size], want[f]), f"filter {f}"
        assert not body[want[f].size:].any(), f"pad of filter {f}"
        low = _get(big, max(0, lo - B32), hi - B32 - max(0, lo - B32))
        assert (low == 0xAB).all(), f"filter {f} wrote 2^32 below its range"


# ================================================================ 5. the 2^31-bit filter boundary
@pytest.fixture(scope="module")
def arena31(dev):
    """2^28 + 64 random bytes on the device, and once on the host for the oracle."""
    g = dev.Generator(device="cuda")
    g.manual_seed(31)
    d = dev.randint(0, 256, ((1 << 28) + 64,), dtype=dev.uint8, device="cuda", generator=g)
    h = d.cpu().numpy()
    yield d, h
    d.untyped_storage().resize_(0)


@pytest.mark.parametrize("bpk", [3, 10])
def test_filter_of_2_31_bits(dev, ab, oracle, arena31, bpk):
    """Filter 0 = [0, 2^28 - 1): m = 2^31 - 8, the largest the reference's
    `int m` holds (src/filter_block.cpp:50); filter 1 = [0, 2^28): 2^31 bits,
    answers 0; filter 2 is an empty range and id 3 is past the last filter.
    Half the arena's bits are set, so with k = 2 (bpk 3) a quarter of filter
    0's queries answer 1 and with k = 6 (bpk 10, pb_bin_kernel<6>) one in 64.
    Nothing is asserted about adl_bloom_probe_device / _probe_multi_device at
    2^31 bits: the header is silent there."""
    d_arena, h_arena = arena31
    top = (1 << 28) - 1
    begin, end = np.array([0, 0, 4096], np.uint64), np.array([top, top + 1, 4096], np.uint64)
    d_begin, d_end = _d(dev, begin), _d(dev, end)
    rng = np.random.default_rng(31)
    n = (1 << 20) + 4097
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    fid = rng.integers(0, 4, n).astype(np.uint32)
    want = np.zeros(n, np.uint8)
    want[fid == 0] = oracle.probe(keys[fid == 0], h_arena[:top], bits_per_key=bpk)
    assert 0 < int(want.sum()) < int((fid == 0).sum()) // 2
    d_keys, d_fid = _d(dev, keys), _d(dev, fid)
    assert np.array_equal(_ranges(dev, ab, d_keys, None, n, 16, d_fid, 3, d_arena, d_begin, d_end, bpk), want)
    assert ab.lib().adl_bloom_probe_batch_workspace_bytes(n, 3, bpk, 16) > 256  # the binned pipeline's plan
    got = ab.probe_batch(d_keys, d_fid, d_arena, d_begin, bits_per_key=bpk, bitmap_end=d_end).cpu().numpy()
    assert np.array_equal(got, want)
    nf = 60_000
    hit0 = oracle.probe(keys[:nf], h_arena[:top], bits_per_key=bpk)
    lists = [[int(fid[i]), (int(fid[i]) + 1) % 4] + ([(int(fid[i]) + 3) % 4] if i % 2 else []) for i in range(nf)]
    got, pf = _fanout(dev, ab, d_keys, None, nf, 16, lists, 3, d_arena, d_begin, d_end, bpk)
    assert np.array_equal(got, np.where(pf == 0, hit0[np.repeat(np.arange(nf), [len(x) for x in lists])], 0))
    # verify: 20 000 keys of filter 0, the first 37 of them keys it holds, then 5 000 of filter 1
    n0, n1, lead = 20_000, 5_000, 37
    h0 = oracle.probe(keys[:n0], h_arena[:top], bits_per_key=bpk)
    order = np.concatenate([np.nonzero(h0)[0][:lead], np.nonzero(h0 == 0)[0], np.nonzero(h0)[0][lead:]])
    assert int(h0.sum()) > lead
    vk = np.concatenate([keys[:n0][order], keys[n0:n0 + n1]])
    missing = int((h0 == 0).sum()) + n1
    got = _verify(dev, ab, _d(dev, vk), None, n0 + n1, 16, [0, n0, n0 + n1, n0 + n1], 3, d_arena, d_begin, d_end, bpk)
    assert got == (missing, lead)


# ================================================================ 6. the launch-group split
def test_build_launch_group_split(dev, ab, oracle, knobs, capfd):
    """bpk 44 (k = 30): a launch group holds at most floor(2^31 / 30) =
    71 582 788 keys, so of the 74 filters [1 000 000] * 72 + [0, 777] the
    first 71 fill group 1 and filters 71-73 are group 2, built from a non-zero
    key_begin in the workspace group 1 has just used, with descriptors of their
    own.  Filter f holds the 1 M-key SplitMix block f % 3, so filters 70 and
    71, on either side of the split, differ; every filter's output range (the
    zero pad and the empty filter's 7 zero bytes included) is compared on the
    device with the oracle's bitmap.  Two launch lines for the one call; with
    the first 71 filters alone (exactly at the limit) one line and the same
    bitmaps.  A workspace one byte short is ADL_ERR_WORKSPACE before anything
    is launched.  adl_bloom_build_positions reads the last group's tables.
    The 74 filters are then built once more from the same keys one byte past
    a 16-byte boundary (fixed-stride keys, hashed from memory key by key):
    group 2 again starts at a non-zero key_begin.

    adl_bloom_filter_block_build_device and the cache builds cannot reach the
    split: a block is capped at 2^31 bytes, fewer keys than the group limit
    for every k.

    On an MI355X adl_bloom_build_workspace_bytes gave 9 167 471 416 bytes (group
    1's plan: 55 664 chunks of 38 280 position words); the output is
    3 168 035 376 bytes, the keys 1 152 012 432; the case took 0.9 s, most of it
    the oracle's four builds."""
    bpk, M = 44, 1_000_000
    counts = [M] * 72 + [0, 777]
    gmax = (1 << 31) // 30
    assert ab.num_probes(bpk) == 30 and 71 * M <= gmax < 72 * M
    seeds = (0x61, 0x62, 0x63, 0x64)
    blocks = [ab.synth_keys16(M, seed=s) for s in seeds[:3]]
    keys = dev.empty((72 * M + 777, 16), dtype=dev.uint8, device="cuda")
    keys[:72 * M].view(24, 3, M, 16)[:] = dev.stack(blocks)
    keys[72 * M:] = ab.synth_keys16(777, seed=seeds[3])
    del blocks
    want = [oracle.keys2block(oracle.splitmix_keys16(s, M), bits_per_key=bpk) for s in seeds[:3]]
    want.append(oracle.keys2block(oracle.splitmix_keys16(seeds[3], 777), bits_per_key=bpk))
    assert want[0].size == 44_000_007
    d_want = [_d(dev, np.concatenate([w, np.zeros(-w.size % 16, np.uint8)])) for w in want]
    kb = _kb(counts)
    alloc = np.array([ab.bitmap_alloc_bytes(c, bpk) for c in counts], np.uint64)
    boff = np.concatenate([[0], np.cumsum(alloc)[:-1]]).astype(np.uint64)
    out = ab.empty_device(int(alloc.sum()))
    wsb = ab.workspace_bytes(counts, bpk)
    with capfd.disabled():
        print(f"\ncase 6: build workspace {wsb} bytes, output {out.numel()} bytes, keys {keys.numel()} bytes")
    assert wsb > B32
    ws = ab.empty_device(wsb)

    def check(nf):
        for f in range(nf):
            got = out[int(boff[f]):int(boff[f] + alloc[f])]
            exp = d_want[f % 3] if f < 72 else (d_want[3] if f == 73 else dev.zeros(16, dtype=dev.uint8, device="cuda"))
            assert dev.equal(got, exp), f"filter {f}"

    _debug(knobs, capfd)
    win = out[:64 << 20]
    win.fill_(0xAB)
    assert _segmented(dev, ab, keys, 16, kb, bpk, out, boff, ws, wsb - 1) == ADL_ERR_WORKSPACE
    assert _launches(capfd) == []
    assert bool((win == 0xAB).all())

    out.fill_(0xAB)
    assert _segmented(dev, ab, keys, 16, kb, bpk, out, boff, ws, wsb) == 0
    lines = _launches(capfd)
    assert len(lines) == 2, lines
    _assert_launch(lines[0], GENERIC, True)    # 71 filters: the FilterTable
    _assert_launch(lines[1], GENERIC, False)   # 3 filters: the kernarg
    check(74)
    cnt = np.array(counts, np.uint64)
    v = ctypes.c_uint64()
    assert ab.lib().adl_bloom_build_positions(cnt.ctypes.data, 74, bpk, _p(ws), ctypes.byref(v), _stream(dev)) == 0
    assert 0 < v.value <= 30 * (M + 777)

    out.fill_(0xAB)
    assert _segmented(dev, ab, keys, 16, kb[:72], bpk, out, boff[:71], ws, wsb) == 0
    lines = _launches(capfd)
    assert len(lines) == 1, lines
    _assert_launch(lines[0], GENERIC, True)
    check(71)
    assert bool((out[int(boff[71]):] == 0xAB).all())

    # the same keys one byte past a 16-byte boundary: the fixed-stride view
    shifted = dev.empty(keys.numel() + 16, dtype=dev.uint8, device="cuda")
    shifted[1:1 + keys.numel()] = keys.view(-1)
    del keys
    out.fill_(0xAB)
    assert _segmented(dev, ab, shifted[1:], 16, kb, bpk, out, boff, ws, wsb) == 0
    lines = _launches(capfd)
    assert len(lines) == 2, lines
    _assert_launch(lines[0], GENERIC, True)
    _assert_launch(lines[1], GENERIC, False)
    check(74)


# ================================================================ 7. a filter cache above 4 GiB
def test_filter_cache_above_4gib(dev, ab, oracle):
    """Three ballast tables of 7 x 268 400 007 bytes (2 684 keys at bpk
    100 000: a filter just under 2^31 bits, trivial to hash) fill the arena's
    first 5.6 GB; the library's own verify (ADL_BLOOM_CACHE_VERIFY) and 100
    member Gets are all that is checked of them.  Tables X (put), Y (host
    build, bpk 3) and Z (device build, bpk 16) then lie above 4 GiB and are
    probed by a launched batch, by the resident server (single-key calls), by
    the fan-out and at filter indices 1-3, each against the oracle with the
    block's own bits_per_key."""
    cache = ab.FilterCache(6 << 30, max_tables=16)
    try:
        NB, BB = 2684, 100_000
        assert ab.bitmap_bytes(NB, BB) == 268_400_007
        for b in range(3):
            oid = b"ballast%d" % b
            keys = ab.synth_keys16(7 * NB, seed=0xBA00 + b)
            t = cache.build_device(keys, np.arange(8) * NB, bits_per_key=BB, flags=ab.CACHE_VERIFY, h_block=None)
            assert cache.publish_status(t, oid) == ab.ADL_OK  # (the library's verify found every key)
            got, unc = cache.probe([oid], np.zeros(100, np.uint32), keys[:100].cpu().numpy())
            assert got.all() and unc == 0
            del t, keys
        # the arena hands out the lowest free range that fits (first fit over an offset-ordered
        # free list), so with 2^32 bytes in use every range reserved from here on lies above 4 GiB
        tables, used = cache.stats()
        assert tables == 3 and used >= B32

        rng = random.Random(7)
        xk = [rng.randbytes(rng.randrange(0, 121)) for _ in range(20_000)]
        xkb = [0, 9000, 9001, 20_000]
        xb = [oracle.keys2block(xk[xkb[f]:xkb[f + 1]]) for f in range(3)]
        xblock = oracle.filter_block_final([b.tobytes() for b in xb], 10)
        cache.put(b"X", xblock)
        yk = oracle.splitmix_keys16(0x77, 9000)
        ykb = [0, 5000, 9000]
        yb = [oracle.keys2block(yk[ykb[f]:ykb[f + 1]], bits_per_key=3) for f in range(2)]
        yblock, t = cache.build(yk, ykb, bits_per_key=3)
        assert yblock == oracle.filter_block_final([b.tobytes() for b in yb], 3)
        cache.publish(t, b"Y")
        zk = ab.synth_keys16(12_000, seed=0x78)
        zb = [oracle.keys2block(zk.cpu().numpy(), bits_per_key=16)]
        t = cache.build_device(zk, [0, 12_000], bits_per_key=16)
        cache.publish(t, b"Z")
        assert t.block_bytes() == oracle.filter_block_final([zb[0].tobytes()], 16)
        assert cache.stats()[0] == 6

        oids = [b"X", b"Y", b"Z", b"not cached"]
        meta = [(xb, 10), (yb, 3), (zb, 16)]
        member = [xk, [bytes(k) for k in yk], [bytes(k) for k in zk.cpu().numpy()]]

        def queries(n):
            """Half of them keys of the table they are bound for (of any of its filters)."""
            table = np.array([rng.randrange(4) for _ in range(n)], np.uint32)
            qs = [rng.choice(member[t]) if t < 3 and rng.random() < 0.5 else rng.randbytes(rng.choice((16, 40)))
                  for t in table]
            return qs, table

        def expect(qs, table, filt=0):
            want = np.ones(len(qs), np.uint8)  # a table that is not cached answers 1
            for t, (bms, bpk) in enumerate(meta):
                sel = np.nonzero(table == t)[0]
                want[sel] = oracle.probe([qs[i] for i in sel], bms[filt], bits_per_key=bpk) if filt < len(bms) else 0
            return want

        qs, table = queries(5000)
        data, offs = oracle.pack(qs)
        want = expect(qs, table)
        assert 0 < int(want[table < 3].sum()) < int((table < 3).sum())
        got, unc = cache.probe(oids, table, data, offs)
        assert np.array_equal(got, want) and unc == int((table == 3).sum())
        for filt in (1, 2, 3):  # X has filters 0-2, Y 0-1, Z 0: a filter the block does not have answers 0
            got, _ = cache.probe(oids, table, data, offs, filter=filt)
            assert np.array_equal(got, expect(qs, table, filt)), filt
        before = ab.probe_server_launches()
        for i in range(300):
            d1, o1 = oracle.pack([qs[i]])
            got, _ = cache.probe(oids, table[i:i + 1], d1, o1)
            assert got[0] == want[i], i
        assert ab.probe_server_launches() > before
        nk = 2000
        lists = [[int(table[i]), (int(table[i]) + 1) % 4] + ([(int(table[i]) + 2) % 4] if i % 2 else [])
                 for i in range(nk)]
        pb = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
        pt = np.concatenate(lists).astype(np.uint32)
        d2, o2 = oracle.pack(qs[:nk])
        got, unc = cache.probe_fanout(oids, pb, pt, d2, o2)
        owner = np.repeat(np.arange(nk), [len(x) for x in lists])
        assert np.array_equal(got, expect([qs[i] for i in owner], pt)) and unc == int((pt == 3).sum())

        # X again, low: the first ballast table's range is the lowest free one
        assert cache.remove(b"ballast0")
        cache.put(b"X2", xblock)
        sel = np.nonzero(table == 0)[0]
        d3, o3 = oracle.pack([qs[i] for i in sel])
        hi, _ = cache.probe([b"X", b"X2"], np.zeros(sel.size, np.uint32), d3, o3)
        lo, _ = cache.probe([b"X", b"X2"], np.ones(sel.size, np.uint32), d3, o3)
        assert np.array_equal(hi, want[sel]) and np.array_equal(lo, want[sel])
    finally:
        cache.close()
