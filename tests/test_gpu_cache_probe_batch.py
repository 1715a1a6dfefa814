"""GPU: the filter cache's bulk probe of device keys
(adl_bloom_filter_cache_probe_batch_device, csrc/filter_cache.hip): the listed
tables resolved and pinned once, then adl_bloom_probe_batch_k_device over the
arena, each table with the k of its own block.

The cache holds blocks written under bits_per_key 3, 10, 16 and 44 (k = 2, 6,
11 and 30); table 1 has two filters, table 4 is listed but never put, and the
queries' table indices come from [0, num_tables + 2).  Every answer equals the
oracle's for its (key, table) -- one oracle.probe_multi per distinct
bits_per_key (tests/mixedk.py), 1 for the table that is not cached, 0 for a
filter the block does not have and for an index past the list -- with `==`,
and FilterCache.probe's (the host call) on the same queries, byte for byte.
After every call, removing every table brings bytes_used to 0: the pins were
given back.
"""
import gc
import re
import threading

import numpy as np
import pytest

import probekeys as pk
from mixedk import MixedBatch, MixedFilters, oracle_answers

pytestmark = pytest.mark.gpu

N = (1 << 20) + 777
VAR_MIN = "ADL_BLOOM_PROBE_BATCH_VAR_MIN"
MAX_K = "ADL_BLOOM_PROBE_BATCH_MAX_K"
LINE = re.compile(r"adl_bloom probe_batch_k: (binned|direct) \(([^)]*)\), kmax=(\d+)")
ADL_ERR_WORKSPACE = -5
UNCACHED = 4
# filter 0 of every listed table: (members, bits_per_key); table 4's block is never put
SPEC0 = [(20_000, 3), (13_200, 10), (5_000, 16), (3_000, 44), (1_000, 10), (4_000, 10)]
# filter 1: table 1 only
SPEC1 = [(None, 3), (500, 10), (None, 16), (None, 44), (None, 10), (None, 10)]
OIDS = [b"table-%d" % t for t in range(len(SPEC0))]


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


@pytest.fixture(autouse=True)
def release(dev, knobs):
    knobs.set(MAX_K, 30)  # whatever the default: the pipeline takes every max_k here
    yield
    gc.collect()
    dev.cuda.synchronize()
    dev.cuda.empty_cache()


def _d(dev, a):
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


class Tables:
    """The blocks of SPEC0 / SPEC1 and two batches, one whose members are members of
    filter 0 of their table and one of filter 1, with the cache's expected answers."""

    def __init__(self, oracle, stride=16, seed=0xC0):
        self.stride = stride
        self.f = [MixedFilters(oracle, SPEC0, seed=seed, stride=stride),
                  MixedFilters(oracle, SPEC1, seed=seed + 1, stride=stride)]
        self.blocks = []
        for t, (_, bpk) in enumerate(SPEC0):
            bms = [self.f[0].bms[t].tobytes()] + ([self.f[1].bms[t].tobytes()] if SPEC1[t][0] is not None else [])
            self.blocks.append(oracle.filter_block_final(bms, bpk))
        lens = None if stride is not None else pk.zipf_lengths(oracle, N, seed + 2)
        self.batch = [MixedBatch(oracle, self.f[j], N, seed=seed + 3 + j, stride=stride, lens=lens) for j in (0, 1)]
        self.want = []
        for j in (0, 1):
            w = self.batch[j].want.copy()
            w[self.batch[j].fid == UNCACHED] = 1  # "may be present"
            w.flags.writeable = False
            self.want.append(w)
        assert not self.want[1][(self.batch[1].fid != 1) & (self.batch[1].fid != UNCACHED)].any()

    def cache(self, ab, capacity=8 << 20):
        c = ab.FilterCache(capacity, max_tables=64)
        for t, oid in enumerate(OIDS):
            if t != UNCACHED:
                c.put(oid, self.blocks[t])
        return c


@pytest.fixture(scope="module")
def tabs(oracle):
    return Tables(oracle)


def drained(cache, oids=OIDS):
    """Removing every table frees the whole arena at once: no pin is left."""
    for oid in oids:
        cache.remove(oid)
    return cache.stats() == (0, 0)


def device_keys(dev, b):
    if b.stride is None:
        return _d(dev, b.data), _d(dev, b.off)
    return _d(dev, b.keys), None


# ---------------------------------------------------------------- 1 answers
@pytest.mark.parametrize("filt", [0, 1])
def test_answers_16_byte_keys(dev, ab, knobs, capfd, tabs, filt):
    """filter 0, and filter 1, which only table 1's block has."""
    b, want = tabs.batch[filt], tabs.want[filt]
    cache = tabs.cache(ab)
    keys, _ = device_keys(dev, b)
    knobs.set("ADL_BLOOM_DEBUG", 1)
    capfd.readouterr()
    out, cached = cache.probe_batch_device(OIDS, _d(dev, b.fid), keys, filter=filt)
    assert LINE.findall(capfd.readouterr().err) == [("binned", "keys16", "30")]
    got = out.cpu().numpy()
    same(got, want, "probe_batch_device")
    assert cached.tolist() == [int(t != UNCACHED) for t in range(len(OIDS))]
    valid = np.nonzero(b.fid < len(OIDS))[0]  # (the host call refuses an index past the list)
    host, unc = cache.probe(OIDS, b.fid[valid], b.keys[valid], filter=filt)
    assert unc == int((b.fid[valid] == UNCACHED).sum())
    assert got[valid].tobytes() == host.tobytes()
    assert not got[b.fid >= len(OIDS)].any()
    assert drained(cache)


def test_answers_varlen_keys(dev, ab, oracle, knobs, capfd):
    """Zipf 8-256 B keys with the knob forced."""
    knobs.set(VAR_MIN, 1)
    tv = Tables(oracle, stride=None, seed=0xD0)
    b, want = tv.batch[0], tv.want[0]
    cache = tv.cache(ab)
    keys, off = device_keys(dev, b)
    knobs.set("ADL_BLOOM_DEBUG", 1)
    capfd.readouterr()
    out, cached = cache.probe_batch_device(OIDS, _d(dev, b.fid), keys, offsets=off)
    assert LINE.findall(capfd.readouterr().err) == [("binned", "var", "30")]
    same(out.cpu().numpy(), want, "probe_batch_device")
    assert cached.tolist() == [int(t != UNCACHED) for t in range(len(OIDS))]
    assert drained(cache)


def test_small_batch_goes_direct(dev, ab, knobs, capfd, tabs):
    n = 5_000
    b, want = tabs.batch[0], tabs.want[0]
    cache = tabs.cache(ab)
    assert cache.probe_batch_workspace_bytes(OIDS, n, 16) == 256
    knobs.set("ADL_BLOOM_DEBUG", 1)
    capfd.readouterr()
    out, cached = cache.probe_batch_device(OIDS, _d(dev, b.fid[:n]), _d(dev, b.keys[:n]))
    assert LINE.findall(capfd.readouterr().err) == [("direct", "stride 16", "30")]
    same(out.cpu().numpy(), want[:n], "probe_batch_device")
    host, _ = cache.probe(OIDS, np.minimum(b.fid[:n], len(OIDS) - 1), b.keys[:n])
    ok = b.fid[:n] < len(OIDS)
    assert out.cpu().numpy()[ok].tobytes() == host[ok].tobytes()
    assert drained(cache)


# ---------------------------------------------------------------- 2 a stale workspace size
def test_workspace_sized_before_a_table_grew_its_k(dev, ab, oracle, tabs):
    """The size is asked while table 5 is a bpk-10 block; the table is then put again as a
    bpk-44 block of the same keys: ADL_ERR_WORKSPACE, d_out untouched, no pin left behind
    (a remove frees the range at once), and asking again succeeds."""
    b = tabs.batch[0]
    f0 = tabs.f[0]
    oids = [OIDS[0], OIDS[5]]
    fid = np.where(b.fid == 5, 1, np.where(b.fid == 0, 0, 2)).astype(np.uint32)  # (2: past the list)
    cache = ab.FilterCache(8 << 20, max_tables=64)
    cache.put(oids[0], tabs.blocks[0])
    cache.put(oids[1], tabs.blocks[5])
    wsb6 = cache.probe_batch_workspace_bytes(oids, N, 16)
    assert wsb6 == ab.lib().adl_bloom_probe_batch_k_workspace_bytes(N, 2, 6, 16)
    o5 = f0.moff[f0.first[5]:f0.first[6] + 1]
    bm44 = oracle.keys2block(f0.data, o5, bits_per_key=44)
    cache.put(oids[1], oracle.filter_block_final([bm44.tobytes()], 44))
    keys, d_fid = _d(dev, b.keys), _d(dev, fid)
    ws = dev.full((wsb6,), 0x5A, dtype=dev.uint8, device="cuda")
    out = dev.full((N,), 0xA5, dtype=dev.uint8, device="cuda")
    rc, _, cached = cache.probe_batch_device_status(oids, d_fid, keys, out=out, workspace=ws)
    assert rc == ADL_ERR_WORKSPACE, rc
    dev.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == 0x5A).all())
    assert cached.tolist() == [1, 1]
    tables, used = cache.stats()
    assert tables == 2
    assert cache.remove(oids[1])
    t2, used2 = cache.stats()
    assert t2 == 1 and used2 < used and used - used2 >= bm44.size  # freed at once: the failed call holds no pin
    # asking again: table 5 is not cached now, every query bound for it answers 1
    rc, got, cached = cache.probe_batch_device_status(oids, d_fid, keys, out=out)
    assert rc == 0 and cached.tolist() == [1, 0]
    arena = np.concatenate([f0.bms[0], bm44, np.zeros(16, np.uint8)])
    off = np.array([0, f0.bms[0].size, f0.bms[0].size + bm44.size], np.uint64)
    want = oracle_answers(oracle, arena, off, [3, 44], b.data, b.off, fid, stride=16)
    w1 = want.copy()
    w1[fid == 1] = 1
    same(got.cpu().numpy(), w1, "table 5 not cached")
    # and with the bpk-44 block back
    cache.put(oids[1], oracle.filter_block_final([bm44.tobytes()], 44))
    assert cache.probe_batch_workspace_bytes(oids, N, 16) == ab.lib().adl_bloom_probe_batch_k_workspace_bytes(N, 2, 30, 16)
    got, cached = cache.probe_batch_device(oids, d_fid, keys)
    assert cached.tolist() == [1, 1]
    same(got.cpu().numpy(), want, "table 5 at bpk 44")
    # the other way round: a workspace sized at k = 30 serves the table put back at bpk 10
    ws30 = dev.empty(cache.probe_batch_workspace_bytes(oids, N, 16), dtype=dev.uint8, device="cuda")
    cache.put(oids[1], tabs.blocks[5])
    rc, got, _ = cache.probe_batch_device_status(oids, d_fid, keys, workspace=ws30)
    assert rc == 0
    arena10 = np.concatenate([f0.bms[0], f0.bms[5], np.zeros(16, np.uint8)])
    off10 = np.array([0, f0.bms[0].size, f0.bms[0].size + f0.bms[5].size], np.uint64)
    same(got.cpu().numpy(), oracle_answers(oracle, arena10, off10, [3, 10], b.data, b.off, fid, stride=16),
         "table 5 back at bpk 10")
    assert drained(cache, oids)


# ---------------------------------------------------------------- 3 eviction under a running probe
def test_eviction_under_running_probes(dev, ab, oracle):
    """One thread puts 12 tables round and round into a cache with room for about 6 while
    another runs three bulk probes over all 12: every status is OK and no member is
    answered 0 (a cached table's filter holds it, a table that is not cached answers 1)."""
    T, per = 12, 20_000
    flt = MixedFilters(oracle, [(per, 10)] * T, seed=0xE0)
    blocks = [oracle.filter_block_final([bm.tobytes()], 10) for bm in flt.bms]
    oids = [b"evict-%d" % t for t in range(T)]
    b = MixedBatch(oracle, flt, N, seed=0xE1)
    cache = ab.FilterCache(6 * (len(blocks[0]) + 4096), max_tables=64)
    for t in range(6):
        cache.put(oids[t], blocks[t])
    keys, d_fid = _d(dev, b.keys), _d(dev, b.fid)
    wsb = ab.lib().adl_bloom_probe_batch_k_workspace_bytes(N, T, 6, 16)  # (every block is k = 6, or not cached: k = 1)
    ws = dev.empty(wsb, dtype=dev.uint8, device="cuda")
    outs = [dev.full((N,), 0xA5, dtype=dev.uint8, device="cuda") for _ in range(3)]
    dev.cuda.synchronize()
    stop, put_rcs, probe_rcs = threading.Event(), [], []

    def putter():
        t = 6
        while not stop.is_set() and len(put_rcs) < 2000:
            put_rcs.append(cache.put_status(oids[t % T], blocks[t % T]))
            t += 1

    def prober():
        try:
            for out in outs:
                rc, _, _ = cache.probe_batch_device_status(oids, d_fid, keys, out=out, workspace=ws)
                probe_rcs.append(rc)
        finally:
            stop.set()

    threads = [threading.Thread(target=putter), threading.Thread(target=prober)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert probe_rcs == [0, 0, 0]
    assert put_rcs and all(rc == 0 for rc in put_rcs)
    for out in outs:
        got = out.cpu().numpy()
        assert got[b.member].all(), "a member was answered 0"
        assert set(np.unique(got).tolist()) <= {0, 1}
        assert not got[b.fid >= T].any()
    assert drained(cache, oids)
