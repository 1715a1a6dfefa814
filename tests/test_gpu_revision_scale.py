"""GPU: the revision multi-get and the read plan (revision_index.hip, the hit
kernels of bloom_probe.hip, read_plan.hip, adl_bloom_revision_multiget and
adl_bloom_revision_read_plan in filter_cache.hip) at the sizes
tests/test_gpu_revision.py and tests/test_gpu_read_plan.py stop short of.

C. beyond one grid (G = CUs x 8 x 256 keys): bloom_probe_fanout_count_kernel
   and hits_expand_kernel take a second block of keys per workgroup and reuse
   their LDS arrays; level_scan_kernel owns several totals per thread behind
   revision_locate_kernel and behind the hit count;
D. more than 4 096 filters: the count kernel reads its filter table from global
   memory, with one bits_per_key and with a k per filter;
E. revisions of 8 192, 8 193, 9 016 and 65 616 tables through a cache: group
   arrays that come back as pieces of their own, three sort passes and the run
   heads behind a real multi-get;
F. a pair total just below, at and above 2^32 over a revision.

Every expectation comes from the oracle (oracle.level_candidates, probe_multi,
keys2block, filter_block_final), from numpy (test_read_plan_cpu.expected_plan)
or from torch references that tests/test_revision_scale_cpu.py holds against
numpy and the oracle on the CPU -- never from another entry point of the
library.  Large batches are drawn from a pool of at most 100 distinct keys
through an index array on the device; outputs are compared where they live.
Every device call writes into guardband.Guarded buffers of exactly the promised
sizes.  Each case prints the path it reached ("reached: ..." lines, pytest -s)
and asserts that it did reach it."""
import ctypes

import numpy as np
import pytest

import guardband as gb
import revisionkeys as rk
from test_gpu_level_index import _expected_answers, _select, _user, ab, dev  # noqa: F401 (ab, dev: fixtures)
from test_gpu_level_index_scale import (GIB, KBLOCK, POOL_MAX, _assert_equal, _case, _device_keys, _edge_pool,
                                        _expect, _i32, _need, _small_pool, device_compare)
from test_gpu_revision import _hits_of, _multiget_revision
from test_read_plan_cpu import expected_plan

pytestmark = pytest.mark.gpu

SEQS = rk.SEQS
FILL32 = 0xA5A5A5A5
LDS_FILTERS = 4096  # kLdsFilters: the most filters whose table bloom_probe_fanout_count_kernel stages in LDS
FIXED_GROUPS = 8192  # the most tables whose group arrays ride with adl_bloom_revision_read_plan's counts


@pytest.fixture(scope="module", autouse=True)
def _peak(dev):
    dev.cuda.reset_peak_memory_stats()
    yield
    print(f"\nreached: peak of torch's device allocations over this file: "
          f"{dev.cuda.max_memory_allocated() / GIB:.2f} GiB")


# ------------------------------------------------------------------ what a case reached
def _grid(torch):
    """The workgroups of a grid_for(num_keys, 256, 8) launch that covers the device."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 8


def _beyond(torch, name):
    G = _grid(torch) * KBLOCK
    return {"G": G, "G+1": G + 1, "G+257": G + 257, "2G+300": 2 * G + 300}.get(name) or int(name)


def _trips(torch, K):
    nblk = -(-K // KBLOCK)
    return -(-nblk // _grid(torch))


def _passes(num_tables):
    bits = max(int(num_tables - 1).bit_length(), 1)
    return 1 if bits <= 8 else -(-bits // 8)


def _reached(torch, case, K, pairs="-", hits="-", groups="-", passes="-", more=""):
    nblk = -(-K // KBLOCK)
    print(f"\nreached: {case}: K={K} nblk={nblk} grid={_grid(torch)} trips={_trips(torch, K)} "
          f"scan_per_thread={-(-nblk // KBLOCK)} pairs={pairs} hits={hits} groups={groups} passes={passes}{more}")


# ------------------------------------------------------------------ guarded calls
class HitsRun:
    """One adl_bloom_probe_fanout_hits_device call into four guarded buffers of exactly the promised sizes."""

    def __init__(self, torch, ab, kp, op, stride, K, pb32, pf32, P, nf, d_bm, d_off, bpk, cap):
        wsb = ab.lib().adl_bloom_probe_fanout_hits_workspace_bytes(K, P)
        self.hb = gb.Guarded((K + 1) * 4, 4, name="hit_begin")
        self.hf = gb.Guarded(cap * 4, 4, name="hit_filter")
        self.nh = gb.Guarded(8, 8, name="num_hits")
        self.ws = gb.Guarded(wsb, 256, name="workspace")
        rc = ab.lib().adl_bloom_probe_fanout_hits_device(kp, op, K, stride, pb32.data_ptr(), pf32.data_ptr(), P, nf,
                                                         d_bm.data_ptr(), d_off.data_ptr(), None, bpk, self.hb.ptr,
                                                         self.hf.ptr, cap, self.nh.ptr, self.ws.ptr, wsb, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        gb.check_all(self.hb, self.hf, self.nh, self.ws)

    @property
    def num_hits(self):
        return int(self.nh.numpy().view(np.uint64)[0])


class PlanRun:
    """One adl_bloom_hits_by_table_device call into five guarded buffers of exactly the promised sizes."""

    def __init__(self, torch, ab, hb32, ht32, K, T, ecap, gcap):
        wsb = ab.lib().adl_bloom_hits_by_table_workspace_bytes(K, ecap, T)
        self.gt = gb.Guarded(gcap * 4, 4, name="group_table")
        self.gbeg = gb.Guarded((gcap + 1) * 4, 4, name="group_begin")
        self.ek = gb.Guarded(ecap * 4, 4, name="entry_key")
        self.counts = gb.Guarded(16, 8, name="counts")
        self.ws = gb.Guarded(wsb, 256, name="workspace")
        rc = ab.lib().adl_bloom_hits_by_table_device(hb32.data_ptr(), ht32.data_ptr(), K, T, self.gt.ptr,
                                                     self.gbeg.ptr, gcap, self.ek.ptr, ecap, self.counts.ptr,
                                                     self.ws.ptr, wsb, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        gb.check_all(self.gt, self.gbeg, self.ek, self.counts, self.ws)

    @property
    def totals(self):
        c = self.counts.numpy().view(np.uint64)
        return int(c[0]), int(c[1])

    @property
    def arrays(self):
        return _i32(self.gt), _i32(self.gbeg), _i32(self.ek)


class RevRun:
    """One adl_bloom_revision_candidates_device call into four guarded buffers of exactly the promised sizes."""

    def __init__(self, torch, ab, rev, kp, op, K, stride, seq, cap):
        wsb = ab.lib().adl_bloom_revision_candidates_workspace_bytes(rev._h, K)
        self.pb = gb.Guarded((K + 1) * 4, 4, name="pair_begin")
        self.pt = gb.Guarded(cap * 4, 4, name="pair_table")
        self.npairs = gb.Guarded(8, 8, name="num_pairs")
        self.ws = gb.Guarded(wsb, 256, name="workspace")
        rc = ab.lib().adl_bloom_revision_candidates_device(rev._h, kp, op, K, stride, seq, self.pb.ptr, self.pt.ptr,
                                                           cap, self.npairs.ptr, self.ws.ptr, wsb, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        gb.check_all(self.pb, self.pt, self.npairs, self.ws)

    @property
    def num_pairs(self):
        return int(self.npairs.numpy().view(np.uint64)[0])


def _dev32(torch, t):
    """An int64 device tensor of u32 values as the int32 tensor the library reads (one spare entry, so that an
    empty array still has an address)."""
    out = torch.zeros(t.numel() + 1, dtype=torch.int32, device="cuda")
    out[:t.numel()] = torch.where(t >= 2**31, t - 2**32, t).to(torch.int32)
    return out


# ------------------------------------------------------------------ C. hits beyond one grid
BEYOND = ("G", "G+1", "G+257", "2G+300")
_filters = {}
_batches = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_batches():
    yield
    _filters.clear()
    _batches.clear()
    _edge.clear()


def _hit_filters(torch, oracle, view):
    """64 keys (16 bytes each for the stride-16 view, 1 to 39 otherwise), 40 filters of bits_per_key 10 built by
    the oracle from subsets of them, and the truth table [pool key, filter] on the device."""
    if view not in _filters:
        stride = 16 if view == "stride16" else None
        rng = np.random.default_rng(40 + (stride or 0))
        pool, bm, off, _ = rk.filters_of_a_pool(oracle, rng, 64, 40, (10,), stride)
        truth = rk.truth_table(oracle, pool, bm, off, 10)
        assert 0 < int(truth.sum()) < 64 * 40
        _filters[view] = {"pool": pool, "stride": stride, "d_bm": torch.from_numpy(bm.copy()).cuda(),
                          "d_off": torch.from_numpy(off.view(np.int64).copy()).cuda(),
                          "truth": torch.from_numpy(truth).cuda()}
    return _filters[view]


def _hits_batch(torch, oracle, K, view):
    """K keys drawn from the pool, 0 to 3 pairs each (a quarter of the keys has none) over the 40 filters, and
    the expected hit arrays (rk.expected_hits), all on the device."""
    if (K, view) not in _batches:
        f = _hit_filters(torch, oracle, view)
        g = torch.Generator(device="cuda")
        g.manual_seed(K * 2 + (view == "var"))
        sel = torch.randint(0, 64, (K,), device="cuda", generator=g)
        cnt = torch.randint(0, 4, (K,), device="cuda", generator=g)
        cnt[-1] = 2  # (K = G + 1: the one key of the second trip has pairs)
        pb = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
        pb[1:] = torch.cumsum(cnt, 0)
        P = int(pb[-1].item())
        pf = torch.randint(0, 40, (P,), device="cuda", generator=g)
        hb, hf, _ = rk.expected_hits(torch, f["truth"], sel, pb, pf)
        _batches[(K, view)] = {"sel": sel, "cnt": cnt, "pb": pb, "pf": pf, "P": P, "hb": hb, "hf": hf}
    return _batches[(K, view)]


def _assert_second_trip(torch, K, cnt, name):
    """The batch does what its name says: K = G is the last size of one trip; every other one takes a second
    block of keys per workgroup, its last block is ragged, and from G + 257 on a block of the second trip holds
    keys without pairs beside keys with pairs."""
    grid = _grid(torch)
    if name == "G":
        assert _trips(torch, K) == 1 and K == grid * KBLOCK
        return
    assert _trips(torch, K) >= 2 and K % KBLOCK != 0, (K, grid)
    if name == "G+1":  # (the second trip is one key)
        return
    second = cnt[grid * KBLOCK:]
    blocks = second[:second.numel() // KBLOCK * KBLOCK].view(-1, KBLOCK)
    mixed = ((blocks == 0).any(1) & (blocks > 0).any(1))
    assert bool(mixed.any().item()), "no block of the second trip has keys without pairs beside keys with pairs"


@pytest.mark.parametrize("view", ("stride16", "var"))
@pytest.mark.parametrize("name", BEYOND)
def test_hits_device_beyond_one_grid(dev, ab, oracle, name, view):
    """bloom_probe_fanout_count_kernel's second block of keys per workgroup (sh1 / sh2 / spb / shits reused),
    level_scan_kernel with several block totals per thread behind it, fanout_compact_kernel over more than
    2 048 workgroups: hit_begin, hit_filter and num_hits exact."""
    torch = dev
    K = _beyond(torch, name)
    f = _hit_filters(torch, oracle, view)
    b = _hits_batch(torch, oracle, K, view)
    _assert_second_trip(torch, K, b["cnt"], name)
    H = b["hf"].numel()
    assert 0 < H < b["P"]
    kp, op, st, keep = _device_keys(torch, f["pool"], b["sel"], f["stride"])
    run = HitsRun(torch, ab, kp, op, st, K, _dev32(torch, b["pb"]), _dev32(torch, b["pf"]), b["P"], 40, f["d_bm"],
                  f["d_off"], 10, H)
    got = run.num_hits
    print(f"num_hits {got}, expected {H}")
    cmp = rk.compare_hits(torch, _i32(run.hb), _i32(run.hf), b["hb"], b["hf"])
    print(cmp)
    assert got == H
    rk.assert_same(cmp, f"K={K} {view}")
    _reached(torch, f"hits beyond one grid {name} {view}", K, pairs=b["P"], hits=H)
    del keep


@pytest.mark.parametrize("T", (40, 300))
@pytest.mark.parametrize("name", BEYOND)
def test_hits_by_table_beyond_one_grid(dev, ab, oracle, name, T):
    """hits_expand_kernel's second block of keys per workgroup, on the EXPECTED hit arrays of the batches above
    (a failure there does not show here): one sort pass (40 tables) and two (300), exact against the torch
    reference where the outputs live, and the same bytes from a second run."""
    torch = dev
    K = _beyond(torch, name)
    b = _hits_batch(torch, oracle, K, "stride16")
    hb, hf = b["hb"], b["hf"]
    hits_per_key = hb[1:] - hb[:-1]
    _assert_second_trip(torch, K, hits_per_key, name)
    want = rk.torch_plan(torch, hb, hf)
    H, G = hf.numel(), want[0].numel()
    assert G == 40 and _passes(T) == (1 if T == 40 else 2)
    hb32, hf32 = _dev32(torch, hb), _dev32(torch, hf)
    first = PlanRun(torch, ab, hb32, hf32, K, T, H, G)
    print(f"counts {first.totals}, expected {(H, G)}")
    cmp = rk.compare_plan(torch, first.arrays, want)
    print(cmp)
    assert first.totals == (H, G)
    rk.assert_same(cmp, f"K={K} T={T}")
    again = PlanRun(torch, ab, hb32, hf32, K, T, H, G)
    assert again.totals == (H, G)
    for a, c, part in zip(first.arrays, again.arrays, ("group_table", "group_begin", "entry_key")):
        assert torch.equal(a, c), f"{part} differs between two runs on the same input"
    _reached(torch, f"hits by table beyond one grid {name}", K, hits=H, groups=G, passes=_passes(T))


# ------------------------------------------------------------------ C. revisions beyond one grid
_levels = {}
_revs = {}
_rev_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for s in list(_scales.values()):
        s.close()
    _scales.clear()
    for r in _revs.values():
        r.close()
    for lv in _levels.values():
        lv.close()
    _revs.clear()
    _levels.clear()
    _rev_cases.clear()


def _level(ab, name):
    if name is None:
        return None
    if name not in _levels:
        tables = rk.tables(name)
        _levels[name] = ab.LevelIndex(tables, oids=[b"%s-%d" % (name.encode(), t) for t in range(len(tables))])
    return _levels[name]


def _rev(ab, shape):
    if shape not in _revs:
        _revs[shape] = ab.Revision([_level(ab, n) for n in rk.REVISIONS[shape]])
    return _revs[shape]


def _rev_case(oracle, shape, stride):
    """{pool, want: {seq: per-pool-key global-id lists}} of a revision: at most POOL_MAX keys, an even sample of
    the levels' small pools (test_gpu_level_index_scale._small_pool: boundaries, their successors, edge keys)."""
    if (shape, stride) not in _rev_cases:
        names = rk.REVISIONS[shape]
        keys = set()
        for n in sorted({n for n in names if rk.tables(n)}):
            keys |= set(_small_pool(rk.tables(n), stride))
        keys = sorted(keys)
        must = [k for k in keys if k.rstrip(b"\0") in (b"\x65", b"")]  # (0x65: every table of t300)
        rest = [k for k in keys if k not in must]
        room = POOL_MAX - len(must)
        pool = sorted(set(must) | ({rest[(i * len(rest)) // room] for i in range(room)} if len(rest) > room
                                   else set(rest)))
        want = {seq: rk.revision_lists(oracle, names, pool, seq) for seq in SEQS}
        assert len(pool) <= POOL_MAX
        assert any(not x for x in want[25]) and any(want[24][i] != want[26][i] for i in range(len(pool)))
        assert len({len(x) for x in want[25]}) >= 3
        _rev_cases[(shape, stride)] = {"pool": pool, "want": want, "dev": {}}
    return _rev_cases[(shape, stride)]


@pytest.mark.parametrize("shape,view", (("five", "var"), ("eight", "stride16")))
@pytest.mark.parametrize("name", ("65537", "200001", "G+257"))
def test_revision_candidates_beyond_65536_keys(dev, ab, oracle, name, shape, view):
    """revision_locate_kernel, level_scan_kernel with 2, 4 and 9 block totals per thread and
    revision_expand_kernel over five levels (an empty and a missing one among them) and over eight: pair_begin
    and the global-id lists exact at seq 24, 25 and 26."""
    torch = dev
    K = _beyond(torch, name)
    stride = 16 if view == "stride16" else None
    case = _rev_case(oracle, shape, stride)
    rev = _rev(ab, shape)
    base = rk.table_base(rk.REVISIONS[shape])
    sel = torch.from_numpy(_select(K, len(case["pool"]), len(name) * 7 + (stride or 0))).cuda()
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, stride)
    nblk = -(-K // KBLOCK)
    assert -(-nblk // KBLOCK) >= 2  # level_scan_kernel: more than one total per thread
    for seq in SEQS:
        len_of, lists = _expect(torch, case, seq)
        exp = device_compare(torch, sel, len_of, lists)
        assert int(lists.max().item()) >= int(base[-2])  # ids of the last level: global, not per level
        run = RevRun(torch, ab, rev, kp, op, K, st, seq, exp["total"])
        print(f"seq {seq}: num_pairs {run.num_pairs}, expected {exp['total']}")
        cmp = device_compare(torch, sel, len_of, lists, _i32(run.pb), _i32(run.pt), chunk=1 << 16)
        print({k: v for k, v in cmp.items() if k != "block_totals"})
        assert run.num_pairs == exp["total"]
        _assert_equal(cmp, f"K={K} {shape} {view} seq={seq}")
        if seq == 25:
            _reached(torch, f"revision candidates {shape} {view} {name}", K, pairs=exp["total"])
    del keep


def _host_keys(pool, sel):
    """The var-len keys pool[sel] as host arrays: (packed uint8 bytes, uint64 offsets[K + 1])."""
    begin, flat = rk.gather_lists([list(k) for k in pool], sel)
    return np.concatenate([flat.astype(np.uint8), np.zeros(1, np.uint8)]), begin.astype(np.uint64)


def _assert_plan(got, want, what):
    for g, w, part in zip(got, want, ("group_table", "group_begin", "entry_key")):
        assert len(g) == len(w), f"{what}: {part} has {len(g)} entries, expected {len(w)}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (f"{what}: {bad.size} entries of {part} differ, the first at {int(bad[0])}: "
                               f"got {int(g[bad[0]])}, want {int(w[bad[0]])}")


def test_cached_calls_beyond_one_grid(dev, ab, oracle):
    """Revision.multiget and Revision.read_plan at K = G + 257 through a cache, on test_gpu_revision's three
    levels (bits_per_key 3, 10 and 44, one table never cached): the hit lists are the oracle's per pool key,
    the plan is numpy's grouping of them."""
    torch = dev
    K = _beyond(torch, "G+257")
    assert _trips(torch, K) == 2
    universe, tabs, split = _multiget_revision(oracle)
    cache = ab.FilterCache(16 << 20, max_tables=16)
    levels = [ab.LevelIndex([tabs[t]["range"] for t in ids], oids=[tabs[t]["oid"] for t in ids]) for ids in split]
    rev = ab.Revision(levels)
    try:
        for t in tabs[:4]:
            cache.put(t["oid"], t["block"])
        cached = [True, True, True, True, False]
        rng = np.random.default_rng(K)
        pool = sorted({universe[int(i)] for i in rng.integers(0, len(universe), 88)} |
                      {_user(t["range"][1]) for t in tabs} | {_user(t["range"][0]) for t in tabs} | {b"", b"\xff" * 41})
        assert len(pool) <= POOL_MAX
        seq = 25
        lists = [[ids[0] + t for ids in split for t in oracle.level_candidates([tabs[g]["range"] for g in ids], k, seq)]
                 for k in pool]
        pbeg, pflat = rk.csr(lists)
        ans = _expected_answers(oracle, tabs, pool, pbeg, pflat, cached)
        hit_lists = [[int(t) for t, a in zip(pflat[pbeg[i]:pbeg[i + 1]], ans[pbeg[i]:pbeg[i + 1]]) if a]
                     for i in range(len(pool))]
        assert 0 < sum(map(len, hit_lists)) < len(pflat) and any(len(h) == 0 < len(x) for h, x in zip(hit_lists, lists))
        sel = _select(K, len(pool), 9)
        data, offs = _host_keys(pool, sel)
        pairs = int(np.array([len(x) for x in lists])[sel].sum())
        want_b, want_t = rk.gather_lists(hit_lists, sel)
        want = expected_plan(want_b, want_t)
        want_unc = int((want_t == 4).sum())
        H, G = len(want_t), len(want[0])
        hb, ht, unc = rev.multiget(cache, data, offs, seq=seq)
        bad = np.flatnonzero(hb != want_b)
        assert bad.size == 0, ("hit_begin", int(bad[0]), int(hb[bad[0]]), int(want_b[bad[0]]))
        bad = np.flatnonzero(ht != want_t) if len(ht) == H else np.array([min(len(ht), H)])
        assert bad.size == 0, ("hit_table", len(ht), H, int(bad[0]))
        assert unc == want_unc and unc > 0
        rc, gt, gbeg, ek, ng, nh, npairs, unc2 = rev.read_plan_status(cache, data, offs, seq=seq)
        print(f"read_plan: rc {rc}, groups {ng}, hits {nh}, pairs {npairs}; expected {G}, {H}, {pairs}")
        assert (rc, ng, nh, npairs, unc2) == (0, G, H, pairs, want_unc)
        _assert_plan((gt, gbeg, ek), want, "K = G + 257")
        _reached(torch, "cached multi-get and read plan G+257", K, pairs=pairs, hits=H, groups=G, passes=_passes(5))
    finally:
        rev.close()
        for lv in levels:
            lv.close()
        cache.close()


# ------------------------------------------------------------------ D. the count kernel's global filter table
_many = {}


def _many_filters(oracle):
    """4 097 filters of bits_per_key 10 over a 64-key pool (filter 4 000 is empty) and their truth tables for
    the first 4 096 and for all of them."""
    if not _many:
        pool, bm, off, _ = rk.filters_of_a_pool(oracle, np.random.default_rng(4097), 64, LDS_FILTERS + 1, (10,), None,
                                                empty=4000)
        _many.update(pool=pool, bm=bm, off=off, truth=rk.truth_table(oracle, pool, bm, off, 10))
    return _many


@pytest.mark.parametrize("F", (LDS_FILTERS, LDS_FILTERS + 1))
def test_count_kernel_filter_table_in_lds_and_in_global_memory(dev, ab, oracle, F):
    """adl_bloom_probe_fanout_hits_device with 4 096 filters (the last size whose table is staged in LDS) and
    with 4 097 (read from global memory), one bits_per_key: 1 000 keys of 0 to 5 pairs over all filters, the
    empty one and ids >= num_filters among them, exact against oracle.probe_multi's truth table."""
    torch = dev
    m = _many_filters(oracle)
    truth = np.concatenate([m["truth"][:, :F], np.zeros((64, 1), np.uint8)], 1)
    K = 1000
    rng = np.random.default_rng(F)
    sel = rng.integers(0, 64, K)
    pb = np.concatenate([[0], np.cumsum(rng.integers(0, 6, K))]).astype(np.int64)
    pf = rng.integers(0, F + 40, int(pb[-1]))
    pf[:6] = [F - 1, F, F + 39, 4000, 0, 2**32 - 1]
    t = [torch.from_numpy(x).cuda() for x in (truth, sel, pb, pf)]
    hb, hf, ans = rk.expected_hits(torch, *t)
    H = hf.numel()
    hit_ids = hf.cpu().numpy()
    assert 0 < H < len(pf) and (hit_ids >= LDS_FILTERS // 2).any() and hit_ids.max() < F and 4000 not in hit_ids
    kp, op, st, keep = _device_keys(torch, m["pool"], t[1], None)
    d_bm = torch.from_numpy(m["bm"].copy()).cuda()
    d_off = torch.from_numpy(m["off"][:F + 1].view(np.int64).copy()).cuda()
    run = HitsRun(torch, ab, kp, op, st, K, _dev32(torch, t[2]), _dev32(torch, t[3]), len(pf), F, d_bm, d_off, 10, H)
    print(f"num_hits {run.num_hits}, expected {H}")
    cmp = rk.compare_hits(torch, _i32(run.hb), _i32(run.hf), hb, hf)
    print(cmp)
    assert run.num_hits == H
    rk.assert_same(cmp, f"{F} filters")
    lds_tab = "off" if F > LDS_FILTERS else "on"
    _reached(torch, f"count kernel, {F} filters, lds_tab={lds_tab}", K, pairs=len(pf), hits=H)
    del keep


# ------------------------------------------------------------------ D, E. many tables through a cache
BPKS = (3, 10, 44)
_scales = {}


class Scale:
    """A revision over a cache: its levels with oids, and blocks of four member keys (bits_per_key 3, 10 and 44
    in turn, built by the oracle) put for the tables of the disjoint level that `cached(i)` names."""

    def __init__(self, ab, oracle, names, cached):
        self.names = names
        self.T = len(rk.tables(names[0]))
        self.total = int(rk.table_base(names)[-1])
        self.levels = [ab.LevelIndex(rk.tables(n), oids=[self.oid(n, t) for t in range(len(rk.tables(n)))])
                       for n in names]
        self.rev = ab.Revision(self.levels)
        self.cache = ab.FilterCache(64 << 20, max_tables=max(self.total, 16))
        self.bpk = np.zeros(self.total, np.int64)  # 0: not cached
        bms, self.blocks = [], {}
        for j, i in enumerate(i for i in range(self.T) if cached(i)):
            self.bpk[i] = BPKS[j % 3]
            bm = oracle.keys2block(self.members(i), bits_per_key=int(self.bpk[i])).tobytes()
            self.blocks[i] = oracle.filter_block_final([bm], int(self.bpk[i]))
            self.cache.put(self.oid(names[0], i), self.blocks[i])
            bms.append(bm)
        self.slot = np.cumsum(self.bpk > 0) - 1  # table -> its filter among the concatenated bitmaps
        self.off = np.concatenate([[0], np.cumsum([len(b) for b in bms])]).astype(np.uint64)
        self.bitmaps = np.frombuffer(b"".join(bms) + bytes(16), np.uint8)
        # (a cache that refuses that many tables would have evicted the first ones)
        assert self.cache.stats()[0] == len(bms), (self.cache.stats(), len(bms))
        assert all(self.oid(names[0], i) in self.cache for i in list(self.blocks)[:3] + list(self.blocks)[-3:])

    @staticmethod
    def oid(name, t):
        return b"%s-%d" % (name.encode(), t)

    @staticmethod
    def members(i):
        return [b"d%06d" % i + x for x in (b"b", b"m", b"p", b"y")]

    def answers(self, oracle, keys, begin, flat):
        """Per pair: 1 for a table that is not cached, else oracle.probe_multi over the concatenated bitmaps."""
        owner = np.repeat(np.arange(len(keys)), np.diff(begin.astype(np.int64)))
        want = np.ones(len(flat), np.uint8)
        for b in BPKS:
            s = np.flatnonzero(self.bpk[flat] == b)
            if len(s):
                want[s] = oracle.probe_multi([keys[int(i)] for i in owner[s]], self.slot[flat[s]], self.bitmaps,
                                             self.off, bits_per_key=b)
        return want

    def close(self):
        self.rev.close()
        for lv in self.levels:
            lv.close()
        self.cache.close()


def _scale(ab, oracle, key, names, cached):
    if key not in _scales:
        _scales[key] = Scale(ab, oracle, names, cached)
    return _scales[key]


@pytest.mark.parametrize("T", (LDS_FILTERS, LDS_FILTERS + 1))
def test_count_kernel_filter_table_with_a_k_per_filter(dev, ab, oracle, T):
    """The count kernel's per-filter k table exists only behind a cache: a one-level revision of 4 096 and of
    4 097 disjoint tables, every one cached, bits_per_key 3, 10 and 44 in turn, 1 000 keys: Revision.multiget's
    hits against oracle.probe_multi with each table's own bits_per_key."""
    torch = dev
    s = Scale(ab, oracle, ("d%d" % T,), lambda i: True)
    try:
        rng = np.random.default_rng(T)
        K = 1000
        tabs = rng.integers(0, T, K)
        tabs[:4] = [0, LDS_FILTERS - 1, T - 1, T // 2]
        kinds = [(b"m", b"n", b"zz", b"b", b"c")[int(x)] for x in rng.integers(0, 5, K)]
        keys = [b"d%06d" % int(t) + k for t, k in zip(tabs, kinds)]
        lists = [[] if k == b"zz" else [int(t)] for t, k in zip(tabs, kinds)]  # ("b", "c": inside the range too)
        for i in rng.choice(K, 40, replace=False):
            assert oracle.level_candidates(rk.tables(s.names[0]), keys[int(i)], 25) == lists[int(i)]
        begin, flat = rk.csr(lists)
        ans = s.answers(oracle, keys, begin, flat)
        want_b, want_t = _hits_of(begin, flat, ans)
        by_bpk = {b: (int((s.bpk[flat] == b).sum()), int(ans[s.bpk[flat] == b].sum())) for b in BPKS}
        print("pairs and hits per bits_per_key:", by_bpk)
        assert all(h > 0 for _, h in by_bpk.values()) and by_bpk[44][1] < by_bpk[44][0]  # members hit, others miss
        data, offs = oracle.pack(keys)
        rc, hb, ht, nh, npairs, unc = s.rev.multiget_status(s.cache, data, offs, seq=25)
        print(f"multiget: rc {rc}, hits {nh}, pairs {npairs}; expected {len(want_t)}, {len(flat)}")
        assert (rc, nh, npairs, unc) == (0, len(want_t), len(flat), 0)
        bad = np.flatnonzero(hb != want_b)
        assert bad.size == 0, ("hit_begin", int(bad[0]), int(hb[bad[0]]), int(want_b[bad[0]]))
        assert np.array_equal(ht, want_t)
        lds_tab = "off" if T > LDS_FILTERS else "on"
        assert s.rev.stats()[1][-1] == T == int((s.bpk > 0).sum())  # num_filters of the count kernel, all with a k
        _reached(torch, f"count kernel, {T} cached tables with k per filter, lds_tab={lds_tab}", K, pairs=len(flat),
                 hits=len(want_t))
    finally:
        s.close()


def _scale_batch(oracle, s, seq, num_m, num_zz, num_pool, seed):
    """A shuffled batch over the revision (dT, t16): an "m" and an "n" key for num_m tables of the disjoint
    level (all of them: in a seeded permutation), num_zz "zz" keys, num_pool keys of t16's pool.
    -> (keys, their global-id lists, the indices of the "d" keys)"""
    T = s.T
    rng = np.random.default_rng(seed)
    tabs = rng.permutation(T)[:num_m]
    if num_m < T:
        tabs[:4] = [0, FIXED_GROUPS, T - 1, 255]
    keys, lists = [], []
    for kind in (b"m", b"n"):
        keys += [rk.disjoint_key(int(i), kind) for i in tabs]
        lists += [rk.scale_list(oracle, T, int(i), kind, seq) for i in tabs]
    zz = rng.integers(0, T, num_zz)
    keys += [rk.disjoint_key(int(i), b"zz") for i in zz]
    lists += [rk.scale_list(oracle, T, int(i), b"zz", seq) for i in zz]
    nd = len(keys)
    p16 = rk.pool(("t16",))
    pool = [k for k in p16 if not k.startswith(b"d")]
    pool = [pool[int(i)] for i in rng.choice(len(pool), num_pool, replace=False)]
    keys += pool
    # (none starts with "d": no candidate in the disjoint level, rk.disjoint_list_of_other; t16's from the oracle)
    lists += [rk.disjoint_list_of_other(k) + [T + t for t in rk.level_list(oracle, "t16", k, seq)] for k in pool]
    order = rng.permutation(len(keys))
    keys, lists = [keys[int(i)] for i in order], [lists[int(i)] for i in order]
    d_idx = np.flatnonzero(order < nd)
    return keys, lists, d_idx


def _oracle_sample(oracle, s, keys, lists, seq, at_least):
    """oracle.level_candidates on both levels for `at_least` distinct positions of the batch: the "m" keys of
    the tables around 256, 8 192 and 65 536 and of the last one, five keys of t16's pool, and random others."""
    T = s.T
    named = {rk.disjoint_key(i, b"m") for i in (0, 255, 256, 257, 8191, 8192, 65535, 65536, T - 1) if i < T}
    idx = [i for i, k in enumerate(keys) if k in named]
    assert len(idx) == len(named)
    idx += [i for i, k in enumerate(keys) if not k.startswith(b"d")][:5]
    rng = np.random.default_rng(T + 1)
    first = {}
    for i, k in enumerate(keys):  # (two "zz" keys of the batch may be the same key: one position of each)
        first.setdefault(k, i)
    rest = np.setdiff1d(sorted(first.values()), idx)
    idx += [int(i) for i in rng.choice(rest, at_least - len(idx), replace=False)]
    assert len({keys[i] for i in idx}) == len(idx) == at_least
    for i in idx:
        got = rk.revision_lists(oracle, s.names, [keys[i]], seq)[0]
        assert got == lists[i], (keys[i], got, lists[i])
    return len(idx)


def _groups_fixed(total, pair_cap):
    """adl_bloom_revision_read_plan's groups_fixed: gcap = min(tables, pair capacity), gcap * 8 <= 64 KiB."""
    return min(total, pair_cap) <= FIXED_GROUPS


def _raw_multiget(ab, s, data, offs, K, seq, hit_capacity, pair_capacity):
    """adl_bloom_revision_multiget into arrays of 0xA5: (rc, hit_begin, hit_table, num_hits, num_pairs, uncached)."""
    hb = np.full(K + 1, FILL32, np.uint32)
    ht = np.full(max(hit_capacity, 1), FILL32, np.uint32)
    n = [ctypes.c_uint64(77) for _ in range(3)]
    rc = ab.lib().adl_bloom_revision_multiget(s.rev._h, s.cache._h, 0, data.ctypes.data, offs.ctypes.data, K, 0, seq,
                                              hb.ctypes.data, ht.ctypes.data, hit_capacity, ctypes.byref(n[0]),
                                              pair_capacity, ctypes.byref(n[1]), ctypes.byref(n[2]), None)
    return rc, hb, ht, n[0].value, n[1].value, n[2].value


def _expected(oracle, s, keys, lists):
    begin, flat = rk.csr(lists)
    ans = s.answers(oracle, keys, begin, flat)
    want_b, want_t = _hits_of(begin, flat, ans)
    return len(flat), want_b, want_t, expected_plan(want_b, want_t), int((s.bpk[want_t] == 0).sum())


def _freed_at_once(s, i=0):
    """cache.remove of a table the refused call had pinned takes it out of stats() at once; it is put back."""
    before = s.cache.stats()
    oid = s.oid(s.names[0], i)
    assert s.cache.remove(oid)
    after = s.cache.stats()
    assert after[0] == before[0] - 1 and after[1] < before[1], (before, after)
    s.cache.put(oid, s.blocks[i])
    assert s.cache.stats() == before


@pytest.mark.parametrize("name", tuple(rk.SCALE_REVISIONS))
def test_many_tables_through_cache(dev, ab, oracle, name):
    """Revision.read_plan and Revision.multiget over 8 192, 8 193, 9 016 and 65 616 tables, every third table of
    the disjoint level cached (bits_per_key 3, 10 and 44 in turn: more than 4 096 filters with a k each), one
    "m" and one "n" key per table, 1 000 "zz" keys and 50 keys of t16's pool: the plan is numpy's grouping of
    the expected hits, with default, exact and short capacities."""
    torch = dev
    names = rk.SCALE_REVISIONS[name]
    seq = 25
    s = _scale(ab, oracle, name, names, lambda i: i % 3 == 0)
    T, total = s.T, s.total
    keys, lists, d_idx = _scale_batch(oracle, s, seq, T, 1000, 50, T)
    K = len(keys)
    checked = _oracle_sample(oracle, s, keys, lists, seq, 100 if T > 60000 else 200)
    P, want_b, want_t, want, want_unc = _expected(oracle, s, keys, lists)
    H, G = len(want_t), len(want[0])
    passes = _passes(total)
    assert 0 < want_unc < H < P
    fixed = _groups_fixed(total, P)  # (the default pair capacity, K * the longest list, is larger still)
    assert fixed == (name == "d8176") and (passes == 3) == (name == "d65600") and passes >= 2
    if T >= 9000:
        assert G > FIXED_GROUPS
    data, offs = oracle.pack(keys)
    rc, gt, gbeg, ek, ng, nh, npairs, unc = s.rev.read_plan_status(s.cache, data, offs, seq=seq)
    print(f"read_plan: rc {rc}, groups {ng}, hits {nh}, pairs {npairs}, uncached {unc}; "
          f"expected {G}, {H}, {P}, {want_unc}")
    assert (rc, ng, nh, npairs) == (0, G, H, P)
    _assert_plan((gt, gbeg, ek), want, name)
    assert unc == want_unc
    # t16's groups are the last ones, and each d key is in every one of the d keys' t16 list
    d16 = sorted(T + t for t in rk.t16_list_of_d(oracle, seq))
    n16 = int((gt >= T).sum())
    assert n16 >= len(d16) and (gt[-n16:] >= T).all() and (gt[:-n16] < T).all() and G - n16 == T
    for g in np.flatnonzero(np.isin(gt, d16)):
        entries = ek[gbeg[g]:gbeg[g + 1]]
        assert np.isin(d_idx, entries).all() and len(entries) >= len(d_idx), int(gt[g])
    assert len(np.flatnonzero(np.isin(gt, d16))) == len(d16)
    hb, ht, unc_m = s.rev.multiget(s.cache, data, offs, seq=seq)
    bad = np.flatnonzero(hb != want_b)
    assert bad.size == 0, ("hit_begin", int(bad[0]), int(hb[bad[0]]), int(want_b[bad[0]]))
    assert np.array_equal(ht, want_t) and unc_m == want_unc
    # exact capacities: the same result
    rc, gt4, gb4, ek4, ng4, nh4, np4, unc4 = s.rev.read_plan_status(s.cache, data, offs, seq=seq, entry_capacity=H,
                                                                    group_capacity=G, pair_capacity=P)
    assert (rc, ng4, nh4, np4, unc4) == (0, G, H, P, want_unc)
    _assert_plan((gt4, gb4, ek4), want, name + ", exact capacities")
    rc, hb4, ht4, nh4, np4, unc4 = s.rev.multiget_status(s.cache, data, offs, seq=seq, hit_capacity=H, pair_capacity=P)
    assert (rc, nh4, np4, unc4) == (0, H, P, want_unc) and np.array_equal(hb4, want_b) and np.array_equal(ht4, want_t)
    # each capacity one short: ADL_ERR_WORKSPACE, the totals the header promises, no array written, no pin kept
    for kw, totals in (({"entry_capacity": H - 1, "group_capacity": G, "pair_capacity": P}, (H, G, P)),
                       ({"entry_capacity": H, "group_capacity": G - 1, "pair_capacity": P}, (H, G, P)),
                       ({"entry_capacity": H, "group_capacity": G, "pair_capacity": P - 1}, (0, 0, P))):
        rc, gt2, gb2, ek2, ng2, nh2, np2, unc2 = s.rev.read_plan_status(s.cache, data, offs, seq=seq, **kw)
        assert rc == ab.ADL_ERR_WORKSPACE and (nh2, ng2, np2) == totals and unc2 == 0, (kw, rc, nh2, ng2, np2)
        assert (gt2 == FILL32).all() and (gb2 == FILL32).all() and (ek2 == FILL32).all(), kw
        _freed_at_once(s)
    offs64 = np.ascontiguousarray(offs, np.uint64)
    rc, hb5, ht5, nh5, np5, unc5 = _raw_multiget(ab, s, data, offs64, K, seq, H - 1, P)
    assert rc == ab.ADL_ERR_WORKSPACE and (nh5, np5, unc5) == (H, P, 0)
    assert np.array_equal(hb5, want_b) and (ht5 == FILL32).all()  # h_hit_begin complete, h_hit_table untouched
    _freed_at_once(s)
    rc, hb6, ht6, nh6, np6, unc6 = _raw_multiget(ab, s, data, offs64, K, seq, H, P - 1)
    assert rc == ab.ADL_ERR_WORKSPACE and (nh6, np6, unc6) == (0, P, 0)
    assert (hb6 == FILL32).all() and (ht6 == FILL32).all()  # nothing else written
    _freed_at_once(s)
    _reached(torch, f"many tables {name}", K, pairs=P, hits=H, groups=G, passes=passes,
             more=f" tables={total} cached={int((s.bpk > 0).sum())} groups_fixed={fixed} oracle_sample={checked}")


def test_unfixed_groups_in_a_single_copy(dev, ab, oracle):
    """(d9000, t16) with 300 keys, an exact entry capacity and a pair capacity of the revision's 9 016 tables:
    everything that comes back fits fetch_count_first's single copy (256 KiB) while the group arrays are not
    fixed.  (groups_fixed looks at min(tables, pair capacity): an exact pair capacity, some 3 400 pairs for 300
    keys, or the default one, 300 * 12, would keep the group arrays fixed.)"""
    torch = dev
    name = "d9000"
    s = _scale(ab, oracle, name, rk.SCALE_REVISIONS[name], lambda i: i % 3 == 0)
    seq = 25
    keys, lists, d_idx = _scale_batch(oracle, s, seq, 120, 40, 20, 300)
    K = len(keys)
    assert K == 300
    P, want_b, want_t, want, want_unc = _expected(oracle, s, keys, lists)
    H, G = len(want_t), len(want[0])
    pair_cap = s.total
    fixed = _groups_fixed(s.total, pair_cap)
    assert not fixed and P <= pair_cap and _groups_fixed(s.total, P) and _groups_fixed(s.total, K * s.rev.stats()[2])
    gcap = min(s.total, pair_cap)
    back = 32 + 256 + (gcap + 1) * 4 + 256 + gcap * 4 + 256 + H * 4 + 256  # counts, group arrays, entries
    assert back <= 256 << 10
    data, offs = oracle.pack(keys)
    rc, gt, gbeg, ek, ng, nh, npairs, unc = s.rev.read_plan_status(s.cache, data, offs, seq=seq, entry_capacity=H,
                                                                   pair_capacity=pair_cap)
    print(f"read_plan: rc {rc}, groups {ng}, hits {nh}, pairs {npairs}; expected {G}, {H}, {P}")
    assert (rc, ng, nh, npairs, unc) == (0, G, H, P, want_unc)
    _assert_plan((gt, gbeg, ek), want, "300 keys")
    _reached(torch, "unfixed groups, one copy", K, pairs=P, hits=H, groups=G, passes=_passes(s.total),
             more=f" tables={s.total} pair_capacity={pair_cap} groups_fixed={fixed} bytes_back<={back}")


# ------------------------------------------------------------------ F. around 2^32 pairs of a revision
_edge = {}
EDGE_SEQ = 25
EDGE_LIST = 600


def _rev_edge(torch, oracle):
    """The 300-table level twice, one-byte keys (0x65: all 600 tables).  sel_below: a pair total in
    [2^32 - 600, 2^32); sel_above = sel_below and one more key of 600 candidates: [2^32, 2^32 + 600).  Made on
    the device as test_gpu_level_index_scale._edge_batches makes its own: one key in 64 is drawn from the whole
    pool, the others are 0x65."""
    if not _edge:
        names = rk.REVISIONS["twice300"]
        pool = _edge_pool()
        case = {"pool": pool, "want": {EDGE_SEQ: rk.revision_lists(oracle, names, pool, EDGE_SEQ)}, "dev": {}}
        level = _case(oracle, "t300", 1, pool=pool, check=False)["want"][EDGE_SEQ]
        assert all(x == y + [300 + t for t in y] for x, y in zip(case["want"][EDGE_SEQ], level))
        len_of, _ = _expect(torch, case, EDGE_SEQ)
        host_len = [len(x) for x in case["want"][EDGE_SEQ]]
        assert host_len[0] == EDGE_LIST and 0 in host_len and any(0 < n < EDGE_LIST for n in host_len)
        K0 = 7_100_000
        h = (torch.arange(K0, dtype=torch.int64, device="cuda") * 2654435761) & 0xFFFFFFFF
        sel = torch.where((h >> 26) == 0, (h >> 4) % len(pool), torch.zeros_like(h))
        t0 = int(len_of[sel].sum().item())
        tail = (2**32 - 1 - t0) // EDGE_LIST
        assert tail > 0
        below = torch.cat([sel, torch.zeros(tail, dtype=torch.int64, device="cuda")])
        _edge.update(case=case, below=below, above=torch.cat([below, torch.zeros(1, dtype=torch.int64, device="cuda")]))
    return _edge


def test_revision_just_below_2_32_pairs_capacity_4096(dev, ab, oracle):
    """*d_num_pairs and all of pair_begin exact (revision_expand_kernel's begin entries close to 2^32), the first
    4 096 table entries exact, nothing written behind them."""
    torch = dev
    e = _rev_edge(torch, oracle)
    case, sel = e["case"], e["below"]
    K = sel.numel()
    len_of, lists = _expect(torch, case, EDGE_SEQ)
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, 1)
    run = RevRun(torch, ab, _rev(ab, "twice300"), kp, op, K, st, EDGE_SEQ, 4096)
    cmp = device_compare(torch, sel, len_of, lists, _i32(run.pb), _i32(run.pt), limit=4096)
    print(f"num_pairs {run.num_pairs}, expected {cmp['total']}")
    assert 2**32 - EDGE_LIST <= cmp["total"] < 2**32
    assert run.num_pairs == cmp["total"]
    _assert_equal(cmp, "capacity 4096")
    _reached(torch, "revision just below 2^32, capacity 4096", K, pairs=cmp["total"])


def test_revision_just_below_2_32_pairs_full_capacity(dev, ab, oracle):
    """The one case that writes pair_table at positions close to 2^32: every entry compared, guard bands intact
    behind entry total - 1."""
    torch = dev
    e = _rev_edge(torch, oracle)
    case, sel = e["case"], e["below"]
    K = sel.numel()
    len_of, lists = _expect(torch, case, EDGE_SEQ)
    total = device_compare(torch, sel, len_of, lists)["total"]
    assert 2**32 - EDGE_LIST <= total < 2**32
    _need(torch, 4 * total + 6 * GIB, "a pair_table of 2^32 - x entries, and the comparison's chunks,")
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, 1)
    run = RevRun(torch, ab, _rev(ab, "twice300"), kp, op, K, st, EDGE_SEQ, total)
    print(f"num_pairs {run.num_pairs}, expected {total}")
    assert run.num_pairs == total
    cmp = device_compare(torch, sel, len_of, lists, _i32(run.pb), _i32(run.pt), chunk=1 << 17)
    _assert_equal(cmp, "full capacity")
    _reached(torch, "revision just below 2^32, full capacity", K, pairs=total)


def test_revision_at_and_above_2_32_pairs(dev, ab, oracle):
    """*d_num_pairs exact as a u64; the first 4 096 entries exact (pair_begin has not wrapped there); all guard
    bands intact.  Nothing is asserted about pair_begin: the header calls it meaningless from 2^32."""
    torch = dev
    e = _rev_edge(torch, oracle)
    case, sel = e["case"], e["above"]
    K = sel.numel()
    len_of, lists = _expect(torch, case, EDGE_SEQ)
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, 1)
    run = RevRun(torch, ab, _rev(ab, "twice300"), kp, op, K, st, EDGE_SEQ, 4096)
    cmp = device_compare(torch, sel, len_of, lists, None, _i32(run.pt), limit=4096)
    print(f"num_pairs {run.num_pairs}, expected {cmp['total']}")
    assert 2**32 <= cmp["total"] < 2**32 + EDGE_LIST
    assert run.num_pairs == cmp["total"]
    _assert_equal(cmp, "capacity 4096")
    _reached(torch, "revision at and above 2^32, capacity 4096", K, pairs=cmp["total"])


@pytest.mark.parametrize("call", ("multiget", "read_plan"))
def test_cached_calls_status_on_both_sides_of_2_32_pairs(dev, ab, oracle, call):
    """adl_bloom_revision_multiget and adl_bloom_revision_read_plan on host copies of the two batches, capacity
    4 096: ADL_ERR_WORKSPACE just below 2^32 and ADL_ERR_TOO_LARGE from 2^32, *num_pairs exact both times, the
    other totals 0, every output array still its 0xA5 fill, and the one cached table, put before the call,
    gone from stats() as soon as it is removed after it (no pin kept)."""
    torch = dev
    e = _rev_edge(torch, oracle)
    case = e["case"]
    rev = _rev(ab, "twice300")
    cache = ab.FilterCache(1 << 20, max_tables=16)
    oid = b"t300-7"  # (test_gpu_revision_scale._level's oid of table 7, in both levels)
    block = oracle.filter_block_final([oracle.keys2block([b"\x65", b"\x66"], bits_per_key=10).tobytes()], 10)
    try:
        host_len = np.array([len(x) for x in case["want"][EDGE_SEQ]], np.int64)
        pool_byte = np.frombuffer(b"".join(case["pool"]), np.uint8)
        for which, status in (("below", ab.ADL_ERR_WORKSPACE), ("above", ab.ADL_ERR_TOO_LARGE)):
            sel = e[which].cpu().numpy()
            K = len(sel)
            keys = pool_byte[sel]
            total = int(host_len[sel].sum())
            assert (total < 2**32) == (which == "below") and abs(total - 2**32) <= EDGE_LIST
            cache.put(oid, block)
            assert cache.stats()[0] == 1
            n = [ctypes.c_uint64(77) for _ in range(4)]
            if call == "multiget":
                arrays = [np.full(K + 1, FILL32, np.uint32), np.full(4096, FILL32, np.uint32)]
                rc = ab.lib().adl_bloom_revision_multiget(rev._h, cache._h, 0, keys.ctypes.data, None, K, 1, EDGE_SEQ,
                                                          arrays[0].ctypes.data, arrays[1].ctypes.data, 4096,
                                                          ctypes.byref(n[0]), 4096, ctypes.byref(n[1]),
                                                          ctypes.byref(n[2]), None)
                got = {"pairs": n[1].value, "hits": n[0].value, "groups": 0, "uncached": n[2].value}
            else:
                arrays = [np.full(4096, FILL32, np.uint32), np.full(4097, FILL32, np.uint32),
                          np.full(4096, FILL32, np.uint32)]
                rc = ab.lib().adl_bloom_revision_read_plan(rev._h, cache._h, 0, keys.ctypes.data, None, K, 1, EDGE_SEQ,
                                                           arrays[0].ctypes.data, arrays[1].ctypes.data, 4096,
                                                           ctypes.byref(n[0]), arrays[2].ctypes.data, 4096,
                                                           ctypes.byref(n[1]), 4096, ctypes.byref(n[2]),
                                                           ctypes.byref(n[3]), None)
                got = {"pairs": n[2].value, "hits": n[1].value, "groups": n[0].value, "uncached": n[3].value}
            print(f"{call} {which}: rc {rc}, {got}; expected status {status}, pairs {total}")
            assert rc == status, (which, rc)
            assert got == {"pairs": total, "hits": 0, "groups": 0, "uncached": 0}, (which, got, total)
            assert all((a == FILL32).all() for a in arrays), which
            assert cache.remove(oid) and cache.stats() == (0, 0), which
            _reached(torch, f"{call} {which} 2^32: status {rc}", K, pairs=total)
    finally:
        cache.close()
