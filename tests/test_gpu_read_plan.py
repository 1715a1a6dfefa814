"""GPU: the read plan -- a multi-get's hits grouped by table on the device
(adlsm-tree_amd/csrc/read_plan.hip, adl_bloom_revision_read_plan in
filter_cache.hip, RevisionReadPlanFilter in level_filter.cpp).

* adl_bloom_hits_by_table_device on synthetic hit arrays against numpy (a
  stable argsort of the ids, np.unique for the groups; test_read_plan_cpu.
  expected_plan): H = 0, 1, 63, 64, 65, E-1, E, E+1, 3E+17 and 300E+5 entries
  (E = HITS_TILE) for 1, 2, 256, 257, 65 536, 65 537 and 2^24+1 tables (one to
  four passes, ids over the whole range and ids that differ only in the top
  digit); all hits in one table, every hit another table, runs of one table
  across a wave and a tile boundary, one key with more hits than two tiles,
  runs of keys without hits; the same input twice gives the same bytes; every
  buffer at exactly its promised size inside guard bands, with entry and group
  capacities one short and exact; ids >= num_tables; no keys;
* its stream order behind a delay on a non-default stream;
* Revision.read_plan through a cache (test_gpu_revision's three levels: mixed
  bits_per_key, one table never cached, one removed mid-test) at 700 and
  20 000 keys against the numpy grouping of the oracle's hits and of
  Revision.multiget's own result; short capacities, released pins, no keys, a
  level without oids; the 300-table level twice with nothing cached;
* bin/read_plan_test: the C++ overload forced onto the device and onto the
  host, and --race."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import guardband as gb
import revisionkeys as rk
import streamorder as so
from test_gpu_level_index import _expected_answers, _select, _user
from test_gpu_revision import _hits_of, _multiget_revision
from test_read_plan_cpu import expected_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_MAX = 2**63 - 1
TABLES = (1, 2, 256, 257, 65536, 65537, 2**24 + 1)
FILL32 = 0xA5A5A5A5


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


def _begin(cnt):
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)


def _synthetic(H, T, seed):
    """(hit_begin, hit_table) of exactly H hits over T tables: keys of 0 to 4 hits, no id twice in a key's list,
    300 keys without hits at both ends; every other key's ids differ only in the top digit of the sort."""
    rng = np.random.default_rng(seed)
    cnt = np.minimum(rng.integers(0, 5, 3 * H + 8), T)
    cum = np.cumsum(cnt)
    K = int(np.searchsorted(cum, H)) + 1 if H else 8
    cnt = cnt[:K].copy() if H else np.zeros(K, np.int64)
    if H:
        cnt[-1] -= int(cum[K - 1]) - H
    cnt = np.concatenate([np.zeros(300, np.int64), cnt, np.zeros(300, np.int64)])
    hb = _begin(cnt)
    assert int(hb[-1]) == H
    bits = max(int(T - 1).bit_length(), 1)
    top = 1 << (8 * ((bits + 7) // 8 - 1))
    step = np.where((np.arange(len(cnt)) % 2 == 1) & ((cnt - 1) * top < T), top, 1)
    room = T - np.maximum(cnt - 1, 0) * step
    first = np.floor(rng.random(len(cnt)) * room).astype(np.int64)
    owner = np.repeat(np.arange(len(cnt)), cnt)
    j = np.arange(H) - hb.astype(np.int64)[owner]
    ht = (first[owner] + j * step[owner]).astype(np.uint32)
    assert H == 0 or int(ht.max()) < T
    return hb, ht


def _dev32(torch, a):
    """A device copy of a uint32 array (one spare entry, so that an empty array still has an address)."""
    return torch.from_numpy(np.concatenate([np.asarray(a, np.uint32), np.zeros(1, np.uint32)]).view(np.int32)).cuda()


def _run(torch, ab, hb, ht, T, ecap=None, gcap=None, want=None):
    """One adl_bloom_hits_by_table_device call into guarded buffers of exactly the promised sizes; the result is
    compared with numpy's as far as the capacities reach.  -> (H, G, raw bytes of the outputs)."""
    want_t, want_b, want_k = expected_plan(hb, ht) if want is None else want
    K, H, G = len(hb) - 1, int(hb[-1]), len(want_t)
    ecap = H if ecap is None else ecap
    gcap = G if gcap is None else gcap
    wsb = ab.lib().adl_bloom_hits_by_table_workspace_bytes(K, ecap, T)
    d_hb, d_ht = _dev32(torch, hb), _dev32(torch, ht)
    gt = gb.Guarded(gcap * 4, 4, name="group_table")
    gbeg = gb.Guarded((gcap + 1) * 4, 4, name="group_begin")
    ek = gb.Guarded(ecap * 4, 4, name="entry_key")
    counts = gb.Guarded(16, 8, name="counts")
    ws = gb.Guarded(wsb, 256, name="workspace")
    rc = ab.lib().adl_bloom_hits_by_table_device(d_hb.data_ptr(), d_ht.data_ptr(), K, T, gt.ptr, gbeg.ptr, gcap,
                                                 ek.ptr, ecap, counts.ptr, ws.ptr, wsb, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    gb.check_all(gt, gbeg, ek, counts, ws)
    c = counts.numpy().view(np.uint64)
    got_t, got_b, got_k = (x.numpy().view(np.uint32) for x in (gt, gbeg, ek))
    print(f"H={H} T={T} ecap={ecap} gcap={gcap}: counts {int(c[0])} / {int(c[1])}, expected {H} / {G}")
    assert int(c[0]) == H
    if H > ecap:  # nothing is grouped: only the hit count means anything
        return H, G, b""
    assert int(c[1]) == G
    m = min(G, gcap)
    assert np.array_equal(got_t[:m], want_t[:m])
    assert np.array_equal(got_b[:min(G, gcap) + 1], want_b[:min(G, gcap) + 1])
    bad = np.flatnonzero(got_k[:H] != want_k)
    assert bad.size == 0, (int(bad[0]), int(got_k[bad[0]]), int(want_k[bad[0]]))
    return H, G, got_t.tobytes() + got_b.tobytes() + got_k.tobytes() + c.tobytes()


@pytest.mark.parametrize("T", TABLES)
def test_hits_by_table_sizes_and_passes(dev, ab, T):
    E = ab.HITS_TILE
    groups = 0
    for H in (0, 1, 63, 64, 65, E - 1, E, E + 1, 3 * E + 17, 300 * E + 5):
        hb, ht = _synthetic(H, T, 1000 + H % 997)
        if H >= 64 and T > 256:  # ids that differ only in a digit above the first are there
            assert len(np.unique(ht >> 8)) > 1 or T <= 257
        groups += _run(dev, ab, hb, ht, T)[1]
    assert groups >= min(T, 100)


def _skews(E):
    """name -> (hit_begin, hit_table, num_tables)"""
    rng = np.random.default_rng(77)
    out = {}
    H = 3 * E + 17
    out["one_table"] = (_begin(np.ones(H, np.int64)), np.full(H, 7, np.uint32), 16)
    out["every_hit_another_table"] = (_begin(np.ones(H, np.int64)), rng.permutation(H).astype(np.uint32), H)
    ht = rng.integers(0, 64, H).astype(np.uint32)
    ht[40:105] = 5                  # 65 hits of one table across the first wave's boundary
    ht[E - 100:E - 100 + E + 1] = 9  # E + 1 hits of one table across two tile boundaries
    out["runs_across_wave_and_tile"] = (_begin(np.ones(H, np.int64)), ht, 64)
    big = 2 * E + 3                  # one key whose list is longer than two tiles
    cnt = np.concatenate([rng.integers(0, 4, 200), [big], rng.integers(0, 4, 200)])
    T = big + 10
    lists = [rng.permutation(T)[:c] for c in cnt]
    out["one_key_longer_than_two_tiles"] = (_begin(cnt), np.concatenate(lists).astype(np.uint32), T)
    cnt = np.zeros(5000, np.int64)   # runs of keys without hits: the first and last 300, and two in the middle
    cnt[300:1500] = rng.integers(1, 4, 1200)
    cnt[2100:2105] = 3
    cnt[4000:4700] = rng.integers(0, 3, 700)
    out["runs_of_keys_without_hits"] = (_begin(cnt), np.concatenate(
        [rng.permutation(300)[:c] for c in cnt]).astype(np.uint32), 300)
    return out


@pytest.mark.parametrize("name", ["one_table", "every_hit_another_table", "runs_across_wave_and_tile",
                                  "one_key_longer_than_two_tiles", "runs_of_keys_without_hits"])
def test_hits_by_table_skews_repeatable(dev, ab, name):
    hb, ht, T = _skews(ab.HITS_TILE)[name]
    want = expected_plan(hb, ht)
    H, G, first = _run(dev, ab, hb, ht, T, want=want)
    assert H > 0 and G == {"one_table": 1, "every_hit_another_table": H}.get(name, G)
    assert _run(dev, ab, hb, ht, T, want=want)[2] == first  # byte for byte the same again


def test_hits_by_table_capacities(dev, ab):
    """Capacities one short: nothing outside the smaller buffers is written (the guard bands), the counts are
    complete; exact capacities suffice (every other case here); generous ones change nothing."""
    E = ab.HITS_TILE
    for T in (200, 70000):
        hb, ht = _synthetic(3 * E + 17, T, 5)
        want = expected_plan(hb, ht)
        H, G = int(hb[-1]), len(want[0])
        assert G > 2
        _run(dev, ab, hb, ht, T, ecap=H - 1, want=want)
        _run(dev, ab, hb, ht, T, ecap=E, want=want)
        _run(dev, ab, hb, ht, T, ecap=0, gcap=0, want=want)
        _run(dev, ab, hb, ht, T, gcap=G - 1, want=want)
        _run(dev, ab, hb, ht, T, gcap=1, want=want)
        _run(dev, ab, hb, ht, T, gcap=0, want=want)
        _run(dev, ab, hb, ht, T, ecap=H + 5000, gcap=G + 300, want=want)


def test_hits_by_table_foreign_ids_and_no_keys(dev, ab):
    """Ids >= num_tables: the call promises nothing about the grouping, but writes nothing outside its outputs
    and workspace and reports H.  No keys: no launch, 0 / 0."""
    torch = dev
    E = ab.HITS_TILE
    hb, ht = _synthetic(2 * E + 9, 2**24 + 1, 9)
    H, K = int(hb[-1]), len(hb) - 1
    for T in (0, 1, 200, 65536):
        wsb = ab.lib().adl_bloom_hits_by_table_workspace_bytes(K, H, T)
        d_hb, d_ht = _dev32(torch, hb), _dev32(torch, ht | np.uint32(0x80000000))
        gt, gbeg, ek = gb.Guarded(40, 4), gb.Guarded(44, 4), gb.Guarded(H * 4, 4)
        counts, ws = gb.Guarded(16, 8), gb.Guarded(wsb, 256)
        assert ab.lib().adl_bloom_hits_by_table_device(d_hb.data_ptr(), d_ht.data_ptr(), K, T, gt.ptr, gbeg.ptr, 10,
                                                       ek.ptr, H, counts.ptr, ws.ptr, wsb, None) == 0
        torch.cuda.synchronize()
        gb.check_all(gt, gbeg, ek, counts, ws)
        assert int(counts.numpy().view(np.uint64)[0]) == H
        assert np.array_equal(np.sort(ek.numpy().view(np.uint32)), np.sort(expected_plan(hb, ht)[2]))  # a permutation
    gbeg, counts = gb.Guarded(4, 4), gb.Guarded(16, 8)
    assert ab.lib().adl_bloom_hits_by_table_device(None, None, 0, 16, None, gbeg.ptr, 0, None, 0, counts.ptr, None, 0,
                                                   None) == 0
    torch.cuda.synchronize()
    gb.check_all(gbeg, counts)
    assert not gbeg.numpy().any() and not counts.numpy().any()


def test_hits_by_table_torch_wrapper(dev, ab):
    torch = dev
    hb, ht = _synthetic(5000, 300, 3)
    want_t, want_b, want_k = expected_plan(hb, ht)
    gt, gbeg, ek, counts = ab.hits_by_table(_dev32(torch, hb)[:len(hb)], _dev32(torch, ht)[:len(ht)], 300)
    torch.cuda.synchronize()
    H, G = (int(x) for x in counts.cpu().numpy())
    assert (H, G) == (5000, len(want_t)) and gt.numel() == 300 and ek.numel() == 5000
    assert np.array_equal(gt.cpu().numpy().view(np.uint32)[:G], want_t)
    assert np.array_equal(gbeg.cpu().numpy().view(np.uint32)[:G + 1], want_b)
    assert np.array_equal(ek.cpu().numpy().view(np.uint32), want_k)


def test_hits_by_table_stream_order(dev, ab):
    """On a delayed non-blocking stream the grouping reads the hit arrays the producer wrote on that stream, its
    outputs are complete when the consumer copies them, and the call returns while the delay still runs."""
    E = ab.HITS_TILE
    T = 300
    hb, ht = _synthetic(2 * E + 100, T, 21)
    K, H = len(hb) - 1, int(hb[-1])
    decoy_hb = _begin(np.diff(hb.astype(np.int64))[::-1])
    decoy_ht = ((ht.astype(np.int64) + 1 + np.arange(H) % 7) % T).astype(np.uint32)
    want_t, want_b, want_k = expected_plan(hb, ht)
    G = len(want_t)
    assert not np.array_equal(expected_plan(decoy_hb, decoy_ht)[2], want_k)
    wsb = ab.lib().adl_bloom_hits_by_table_workspace_bytes(K, H, T)
    case = so.Case()
    d_hb, d_ht = case.input(hb, decoy_hb), case.input(ht, decoy_ht)
    gt, gbeg, ek, counts = case.output(T * 4), case.output((T + 1) * 4), case.output(H * 4), case.output(16)
    ws = case.workspace(wsb)

    def entry(stream):
        rc = ab.lib().adl_bloom_hits_by_table_device(d_hb.data_ptr(), d_ht.data_ptr(), K, T, gt.data_ptr(),
                                                     gbeg.data_ptr(), T, ek.data_ptr(), H, counts.data_ptr(),
                                                     ws.data_ptr(), wsb, so.sptr(stream))
        assert rc == 0, rc

    case.run(entry)
    assert case.returned_early, "the call came back only after the delay: it waits for the stream"
    so.check(case.result(counts), np.array([H, G], np.uint64), "counts")
    so.check(case.result(gt, 4 * G), want_t, "group_table")
    so.check(case.result(gbeg, 4 * (G + 1)), want_b, "group_begin")
    so.check(case.result(ek), want_k, "entry_key")
    so.release_delay()


# ------------------------------------------------------------------ Revision.read_plan through a cache
def _assert_plan(got, want, what):
    for g, w, part in zip(got, want, ("group_table", "group_begin", "entry_key")):
        assert np.array_equal(g, w), (what, part)


@pytest.mark.parametrize("K", [700, 20000], ids=["one_copy", "two_phase"])
def test_revision_read_plan_through_cache(dev, ab, oracle, K):
    universe, tabs, split = _multiget_revision(oracle)
    cache = ab.FilterCache(16 << 20, max_tables=16)
    levels = [ab.LevelIndex([tabs[t]["range"] for t in ids], oids=[tabs[t]["oid"] for t in ids]) for ids in split]
    rev = ab.Revision(levels)
    try:
        for t in tabs[:4]:
            cache.put(t["oid"], t["block"])
        cached = [True, True, True, True, False]
        rng = np.random.default_rng(K)
        pool = [universe[int(i)] for i in rng.integers(0, len(universe), 1500)]
        pool += [_user(t["range"][1]) for t in tabs] + [_user(t["range"][0]) for t in tabs] + [b"", b"\xff" * 41]
        keys = [pool[int(i)] for i in _select(K, len(pool), 9)]
        data, offs = oracle.pack(keys)
        memo = {}
        for step, seq in enumerate((25, SEQ_MAX)):
            if step == 1:
                assert cache.remove(tabs[2]["oid"])  # evicted mid-test: answers 1 from now on
                cached[2] = False
            lists = []
            for k in keys:
                if (k, seq) not in memo:
                    memo[(k, seq)] = [ids[0] + t for ids in split
                                      for t in oracle.level_candidates([tabs[g]["range"] for g in ids], k, seq)]
                lists.append(memo[(k, seq)])
            begin, flat = rk.csr(lists)
            want_b, want_t = _hits_of(begin, flat, _expected_answers(oracle, tabs, keys, begin, flat, cached))
            want = expected_plan(want_b, want_t)
            want_unc = int(sum(not cached[int(t)] for t in want_t))
            H, G = len(want_t), len(want[0])
            assert 3 <= G <= 5 and 0 < H < len(flat)
            gt, gbeg, ek, unc = rev.read_plan(cache, data, offs, seq=seq)
            _assert_plan((gt, gbeg, ek), want, "the oracle's hits")
            assert unc == want_unc and unc > 0
            # ... and the numpy grouping of the key-major call's own result
            hb, ht, unc_m = rev.multiget(cache, data, offs, seq=seq)
            _assert_plan((gt, gbeg, ek), expected_plan(hb, ht), "multiget's hits")
            assert unc == unc_m
            # short capacities: ADL_ERR_WORKSPACE, the counts reported, the arrays untouched
            for kw in ({"entry_capacity": H - 1}, {"group_capacity": G - 1}):
                rc, gt2, gb2, ek2, ng2, nh2, np2, unc2 = rev.read_plan_status(cache, data, offs, seq=seq, **kw)
                assert rc == ab.ADL_ERR_WORKSPACE and (nh2, ng2, np2) == (H, G, len(flat)) and unc2 == 0, kw
                assert (gt2 == FILL32).all() and (gb2 == FILL32).all() and (ek2 == FILL32).all()
            rc, gt3, gb3, ek3, ng3, nh3, np3, _ = rev.read_plan_status(cache, data, offs, seq=seq,
                                                                        pair_capacity=len(flat) - 1)
            assert rc == ab.ADL_ERR_WORKSPACE and np3 == len(flat) and (nh3, ng3) == (0, 0)
            assert (gt3 == FILL32).all() and (gb3 == FILL32).all() and (ek3 == FILL32).all()
            # exact capacities are enough
            rc, gt4, gb4, ek4, ng4, nh4, np4, unc4 = rev.read_plan_status(
                cache, data, offs, seq=seq, entry_capacity=H, group_capacity=G, pair_capacity=len(flat))
            assert rc == 0 and (nh4, ng4, np4, unc4) == (H, G, len(flat), want_unc)
            _assert_plan((gt4, gb4, ek4), want, "exact capacities")
            # filter 1 on blocks of one filter: no hit from a cached table
            gt5, gb5, ek5, unc5 = rev.read_plan(cache, data, offs, seq=seq, filter=1)
            assert unc5 == want_unc == len(ek5) and not any(cached[int(t)] for t in gt5)
        # no keys: nothing to do
        rc, gt6, gb6, ek6, ng6, nh6, np6, _ = rev.read_plan_status(cache, np.zeros((0, 16), np.uint8))
        assert rc == 0 and (ng6, nh6, np6) == (0, 0, 0) and list(gb6) == [0] and len(gt6) == 0 and len(ek6) == 0
        # a level created without oids selects but cannot multi-get
        bare_lv = ab.LevelIndex([tabs[t]["range"] for t in split[0]])
        bare = ab.Revision([bare_lv])
        assert bare.read_plan_status(cache, data, offs)[0] == -1
        bare.close()
        bare_lv.close()
    finally:
        rev.close()
        for lv in levels:
            lv.close()
        cache.close()


def test_revision_read_plan_short_capacities_release_their_pins(dev, ab, oracle):
    """adl_bloom_revision_read_plan returning ADL_ERR_WORKSPACE, for too few entries, groups and pairs, has
    unpinned every level's tables: removed right after, they are gone from stats() at once."""
    _, tabs, split = _multiget_revision(oracle)
    tabs, split = tabs[:4], split[:2]
    oids = [t["oid"] for t in tabs]
    keys = [t["members"][i] for t in tabs for i in (100, 500)]  # 8 keys, each inside its table's range
    data, offs = oracle.pack(keys)
    cache = ab.FilterCache(16 << 20, max_tables=16)
    levels = [ab.LevelIndex([tabs[t]["range"] for t in ids], oids=[oids[t] for t in ids]) for ids in split]
    rev = ab.Revision(levels)
    try:
        for t in tabs:
            cache.put(t["oid"], t["block"])
        rc, _, _, _, ng, nh, npairs, _ = rev.read_plan_status(cache, data, offs, entry_capacity=1)
        assert rc == ab.ADL_ERR_WORKSPACE and npairs >= nh >= len(keys) and 1 < ng <= 4
        assert rev.read_plan_status(cache, data, offs, group_capacity=1)[0] == ab.ADL_ERR_WORKSPACE
        rc, _, _, _, _, _, np2, _ = rev.read_plan_status(cache, data, offs, pair_capacity=1)
        assert rc == ab.ADL_ERR_WORKSPACE and np2 == npairs
        assert all(cache.remove(o) for o in oids)
        assert cache.stats() == (0, 0)
        for t in tabs:
            cache.put(t["oid"], t["block"])
        gt, gbeg, ek, unc = rev.read_plan(cache, data, offs)
        hb, ht, _ = rev.multiget(cache, data, offs)
        _assert_plan((gt, gbeg, ek), expected_plan(hb, ht), "after the refusals")
        assert len(ek) == nh and len(gt) == ng and unc == 0
    finally:
        rev.close()
        for lv in levels:
            lv.close()
        cache.close()


def test_revision_read_plan_nothing_cached_600_groups(dev, ab, oracle):
    """The 300-table level twice, nothing cached: every candidate is a hit, one key appears in 600 groups, and
    the sort needs two passes."""
    names = rk.REVISIONS["twice300"]
    keys = rk.pool(names)
    lists = rk.revision_lists(oracle, names, keys, 26)
    begin, flat = rk.csr(lists)
    assert max(len(x) for x in lists) == 600
    want = expected_plan(begin, flat)
    cache = ab.FilterCache(1 << 20, max_tables=16)
    levels = [ab.LevelIndex(rk.tables(n), oids=[b"%d-%d" % (l, t) for t in range(len(rk.tables(n)))])
              for l, n in enumerate(names)]
    rev = ab.Revision(levels)
    try:
        data, offs = oracle.pack(keys)
        gt, gbeg, ek, unc = rev.read_plan(cache, data, offs, seq=26)
        _assert_plan((gt, gbeg, ek), want, "every candidate")
        assert unc == len(flat) and len(gt) == 600
        hot = int(np.argmax([len(x) for x in lists]))
        assert int((ek == hot).sum()) == 600
    finally:
        rev.close()
        for lv in levels:
            lv.close()
        cache.close()


def test_read_plan_binary(dev):
    """bin/read_plan_test: RevisionReadPlanFilter with the threshold forced to the device call and to the host
    grouping equals GroupHitsByTable(RevisionMultiGetFilter(...)) on a three-level revision; --race: four
    threads on one revision and cache, each plan equal to the sequential one."""
    exe = os.path.join(ROOT, "adlsm-tree_amd", "bin", "read_plan_test")
    assert os.path.exists(exe), f"{exe} is missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items()
           if k not in ("ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS", "ADL_BLOOM_REVISION_DEVICE_MIN_KEYS")}
    for mode in ("device", "host", "--race"):
        r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (mode, r.stdout + r.stderr)
        assert " 0 mismatches" in r.stdout, (mode, r.stdout)
