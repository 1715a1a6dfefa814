"""GPU: the resident level index (adlsm-tree_amd/csrc/level_index.hip).

* adl_bloom_level_candidates_device -- locate, scan and expand kernels --
  against oracle.level_candidates (src/revision.cpp:278-287 restated): the
  begin array and the table lists compared exactly, per key, over key counts
  around the 256-key workgroup, levels of 1, 3, 16 and 300 overlapping tables
  (one key with 300 candidates: more than a workgroup) and a 2 000-table
  disjoint level (4 000 boundaries: past the 512 whose prefixes are staged in
  LDS; levels of exactly 512 and of 514 boundaries too), at sequence numbers below, at and above the tables' max seqs, through
  var-len offsets, stride 16, stride 24 and an unaligned base;
* a pair capacity smaller than needed, in guard bands; stream order behind a
  delay on a non-default stream; the torch wrapper;
* adl_bloom_level_multiget through a cache of blocks of bits_per_key 3, 10 and
  44 with one table never cached and one removed mid-test: lists, answers
  (oracle.probe_multi and adl_bloom_filter_cache_probe_fanout on the same
  lists, byte for byte), the uncached count and ADL_ERR_WORKSPACE;
* bin/level_index_test: the C++ overload on both sides of its threshold
  against LevelMultiGetFilter(cache, tables, ...).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import guardband as gb
import streamorder as so
from levelkeys import P40, inner, max_tail as _max_tail, special_users as _special_users

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 255, 256, 257, 1000)
LEVELS = ("t1", "t3", "t16", "t300", "t2000")
EDGE_LEVELS = ("t256", "t257")  # 512 boundaries: the most whose prefixes are staged in LDS; 514: the fewest that are not
VIEWS = ("var", "stride16", "stride24", "unaligned")
SEQS = (24, 25, 26)  # the tables' max seqs are 24, 25 (op 0 and op 1) and 26
SEQ_MAX = 2**63 - 1


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



def _level(name):
    """[(min_inner, max_inner)] in the order handed to the index."""
    rng = np.random.default_rng((LEVELS + EDGE_LEVELS).index(name) + 5)
    sp = _special_users()
    if name == "t1":
        return [(inner(P40, 9, 0), inner(P40, 25, 1))]  # min == max: one boundary
    if name == "t3":
        return [(inner(b"ab", 30, 0), inner(b"ab\0", 25, 1)), (inner(P40[:16], 3, 0), inner(P40 + b"\x80tail", 25, 0)),
                (inner(b"\x7f\x10", 7, 1), inner(b"\x80\x01", 26, 0))]
    if name == "t16":
        tabs = []
        for i in range(16):
            a, b = sorted(int(x) for x in rng.integers(0, len(sp), 2))
            tabs.append((inner(sp[a], int(rng.integers(0, 50)), int(rng.integers(0, 2))), inner(sp[b], *_max_tail(i))))
        tabs[5] = (b"ab", b"\xfe\x80")  # shorter than 9 bytes: (user, seq 0, op 0)
        tabs[7] = (inner(sp[-1], 1, 0), inner(sp[0], 25, 0))  # max < min: never a candidate
        return tabs
    if name == "t300":
        # every min below every max: all 300 overlap between the last min and the first max
        lows = sorted({bytes(rng.integers(0, 0x60, int(rng.integers(1, 30)), dtype=np.uint8)) for _ in range(400)})[:300]
        highs = sorted({b"\x70" + bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8))
                        for _ in range(400)})[:300]
        order = rng.permutation(300)
        return [(inner(lows[int(order[i])], int(rng.integers(0, 50)), 0), inner(highs[i], *_max_tail(i)))
                for i in range(300)]
    # t2000 (t256, t257): disjoint, 4 000 (512, 514) distinct boundaries, many sharing a 20-byte
    # prefix; handed over in descending order
    T = int(name[1:])
    users = set(sp)
    while len(users) < 2 * T:
        n = int(rng.integers(1, 50))
        body = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        users.add((b"shared-prefix-20-byte" if len(users) % 3 == 0 else b"") + body)
    users = sorted(users)
    tabs = [(inner(users[2 * i], 9, 0), inner(users[2 * i + 1], *_max_tail(i))) for i in range(T)]
    return tabs[::-1]


def _user(k):
    return k[:-9] if len(k) >= 9 else k


def _pool(tables, stride):
    """Distinct lookup keys aimed at the level's boundaries.  stride: None for
    var-len keys of 0 to 300 bytes, else every key padded / cut to it."""
    rng = np.random.default_rng(len(tables))
    users = sorted({_user(t[0]) for t in tables} | {_user(t[1]) for t in tables})
    npick = 40 if len(users) <= 1000 else 15  # (the oracle sorts the level once per key)
    pick = users if len(users) <= npick else [users[int(i)] for i in rng.choice(len(users), npick, replace=False)]
    pick = list(pick) + [_user(tables[0][0]), _user(tables[0][1]), _user(tables[-1][1])]
    keys = {b"", b"ab", b"ab\0", b"a", b"\xff\xff\xff", b"\x7f", b"\x80", P40[:16], P40[:17], P40, P40 + b"\x7f",
            bytes(300), b"\xff" * 300, b"\x65"}  # (0x65: between t300's mins and maxes, all 300 tables)
    for u in pick:
        keys |= {u, u + b"\0", u + b"\x80", u[:-1], u[:16] + b"\x01", u[:17] + b"\xee", u[:40] + b"\x05"}
        if u:
            keys |= {u[:-1] + bytes([(u[-1] + 1) & 0xFF]), u[:-1] + bytes([(u[-1] - 1) & 0xFF])}
    for n in (1, 7, 15, 16, 17, 33, 120, 300):
        keys.add(bytes(rng.integers(0, 256, n, dtype=np.uint8)))
    if stride is not None:
        keys = {(k + bytes(stride))[:stride] for k in keys} | {u for u in users[:200] if len(u) == stride}
    return sorted(keys)


def _check_pool(tables, pool, want):
    """The inputs do hold what the comparison has to get right (checked once,
    on the 16-table level's var-len pool, when the fixture is made)."""
    assert b"" in pool and b"ab" in pool and b"ab\0" in pool
    assert {len(k) for k in pool} >= {0, 16, 17, 300}
    users = {_user(t[0]) for t in tables} | {_user(t[1]) for t in tables}
    assert any(k in users for k in pool)
    # a key whose list depends on seq (a table's max user key), and keys without candidates
    assert any(want[24][i] != want[26][i] for i in range(len(pool)))
    assert any(not want[25][i] for i in range(len(pool))) and any(want[25][i] for i in range(len(pool)))
    # signed bytes would order these the other way
    sp = _special_users()
    assert sp.index(b"\x7f\xff\x01") < sp.index(b"\x80\x01")
    assert sorted(sp, key=lambda k: [b - 256 if b >= 128 else b for b in k]) != sp


_cache = {}


def _case(oracle, level, view):
    """(tables, pool, {seq: per-pool-key oracle list}) computed once per (level, view kind)."""
    stride = {"stride16": 16, "stride24": 24}.get(view)
    key = (level, stride)
    if key not in _cache:
        tables = _level(level)
        pool = _pool(tables, stride)
        want = {seq: [oracle.level_candidates(tables, k, seq) for k in pool] for seq in SEQS}
        if key == ("t16", None):
            _check_pool(tables, pool, want)
        _cache[key] = (tables, pool, want)
    return _cache[key]


_levels = {}


@pytest.fixture(scope="module", autouse=True)
def _close_levels():
    yield
    for lv in _levels.values():
        lv.close()
    _levels.clear()


def _index(ab, level):
    if level not in _levels:
        _levels[level] = ab.LevelIndex(_level(level))
    return _levels[level]


def _select(K, npool, seed):
    """K pool indices: the whole pool first (when it fits), the rest random."""
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, npool, K)
    m = min(K, npool)
    sel[:m] = rng.permutation(npool)[:m]
    return sel


def _device_keys(torch, view, keys):
    """-> (key pointer, offsets pointer | None, stride, things to keep alive)."""
    data = np.frombuffer(b"".join(keys), np.uint8)
    if view in ("stride16", "stride24"):
        p = gb.Poisoned(data, 16)  # 16-byte aligned, 0xFF around the keys
        return p.ptr, None, len(keys[0]), (p,)
    p = gb.Poisoned(data, 16, skew=3 if view == "unaligned" else 0)
    offs = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    d_offs = torch.from_numpy(offs).cuda()
    return p.ptr, d_offs.data_ptr(), 0, (p, d_offs)


def _run_select(torch, ab, lv, view, keys, seq, cap):
    """One adl_bloom_level_candidates_device call into guarded buffers: (begin, table[:cap], num_pairs)."""
    K = len(keys)
    kp, op, stride, keep = _device_keys(torch, view, keys)
    wsb = ab.lib().adl_bloom_level_candidates_workspace_bytes(K)
    pb = gb.Guarded((K + 1) * 4, 4, name="pair_begin")
    pt = gb.Guarded(cap * 4, 4, name="pair_table")
    npairs = gb.Guarded(8, 8, name="num_pairs")
    ws = gb.Guarded(wsb, 256, name="workspace")
    rc = ab.lib().adl_bloom_level_candidates_device(lv._h, kp, op, K, stride, seq, pb.ptr, pt.ptr, cap, npairs.ptr,
                                                    ws.ptr, wsb, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    gb.check_all(pb, pt, npairs, ws)
    del keep
    return pb.numpy().view(np.uint32), pt.numpy().view(np.uint32), int(npairs.numpy().view(np.uint64)[0])


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("K", KS)
def test_candidates_device_vs_oracle(dev, ab, oracle, K, level, view):
    torch = dev
    tables, pool, want = _case(oracle, level, view)
    lv = _index(ab, level)
    longest = lv.stats()[3]
    sel = _select(K, len(pool), KS.index(K) * 100 + LEVELS.index(level) * 10 + VIEWS.index(view))
    keys = [pool[int(i)] for i in sel]
    nonempty = 0
    for seq in SEQS:
        lists = [want[seq][int(i)] for i in sel]
        begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
        total = int(begin[-1])
        assert max((len(x) for x in lists), default=0) <= longest
        got_b, got_t, got_n = _run_select(torch, ab, lv, view, keys, seq, max(total, 1))
        assert got_n == total, (seq, got_n, total)
        assert np.array_equal(got_b, begin), (seq, int(np.flatnonzero(got_b != begin)[0]))
        for i, x in enumerate(lists):
            assert list(got_t[begin[i]:begin[i + 1]]) == x, (seq, i, keys[i])
        nonempty += total
    # (t1's one boundary is 40 bytes long: only a var-len key can equal it)
    if K >= 255 and (level != "t1" or view in ("var", "unaligned")):
        assert nonempty > 0
        if level == "t300":
            assert max(len(x) for x in want[26]) == 300  # one key with more candidates than a workgroup has lanes


@pytest.mark.parametrize("level", EDGE_LEVELS)
def test_candidates_device_at_the_lds_staging_limit(dev, ab, oracle, level):
    """Exactly 512 boundaries (all staged in LDS, the last slot used) and 514
    (none staged): every boundary, its neighbours and keys beyond both ends."""
    torch = dev
    tables = _level(level)
    lv = _index(ab, level)
    assert lv.stats()[0] == 2 * 2 * len(tables) + 1  # regions = 2 NB + 1
    users = sorted({_user(t[0]) for t in tables} | {_user(t[1]) for t in tables})
    keys = sorted(set(users) | {u + b"\0" for u in users[::7]} | {u[:-1] for u in users[::5]} | {b"", b"\xff" * 60})
    for seq in (24, 26):
        lists = [oracle.level_candidates(tables, k, seq) for k in keys]
        begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
        flat = np.array([t for x in lists for t in x], np.uint32)
        got_b, got_t, got_n = _run_select(torch, ab, lv, "var", keys, seq, len(flat))
        assert got_n == len(flat) and np.array_equal(got_b, begin) and np.array_equal(got_t, flat)
        # the first boundary (the empty key) is found, and nothing lies beyond the last
        assert lists[keys.index(users[0])] and keys[-1] > users[-1] and not lists[-1]


def test_candidates_device_torch_wrapper(dev, ab, oracle):
    """adlbloom.LevelIndex.candidates_device on torch tensors: the default
    capacity (keys x longest list) and an explicit, smaller one."""
    torch = dev
    tables, pool, want = _case(oracle, "t16", "stride16")
    lv = _index(ab, "t16")
    keys = pool[:300]
    lists = [want[25][i] for i in range(len(keys))]
    begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    flat = np.array([t for x in lists for t in x], np.uint32)
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 16).copy()).cuda()
    pb, pt, n = lv.candidates_device(d_keys, seq=25)
    torch.cuda.synchronize()
    assert int(n.item()) == len(flat) and pt.numel() == len(keys) * lv.stats()[3]
    assert np.array_equal(pb.cpu().numpy().view(np.uint32), begin)
    assert np.array_equal(pt.cpu().numpy().view(np.uint32)[:len(flat)], flat)
    pb, pt, n = lv.candidates_device(d_keys, seq=25, pair_capacity=len(flat) // 2)
    torch.cuda.synchronize()
    assert int(n.item()) == len(flat) and np.array_equal(pb.cpu().numpy().view(np.uint32), begin)
    assert np.array_equal(pt.cpu().numpy().view(np.uint32), flat[:len(flat) // 2])


def test_pair_capacity_smaller_than_needed(dev, ab, oracle):
    """begin complete, *d_num_pairs exact, the first `cap` entries right and
    nothing written past them (the table buffer is exactly cap entries inside
    guard bands)."""
    torch = dev
    for level, K in (("t16", 1000), ("t300", 257)):
        tables, pool, want = _case(oracle, level, "var")
        lv = _index(ab, level)
        sel = _select(K, len(pool), 77)
        keys = [pool[int(i)] for i in sel]
        lists = [want[25][int(i)] for i in sel]
        begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
        total = int(begin[-1])
        flat = np.array([t for x in lists for t in x], np.uint32)
        for cap in (total // 2, 1, total - 1):
            got_b, got_t, got_n = _run_select(torch, ab, lv, "var", keys, 25, cap)
            assert got_n == total and np.array_equal(got_b, begin)
            assert np.array_equal(got_t, flat[:cap]), cap


def test_zero_keys_and_zero_capacity(dev, ab, oracle):
    torch = dev
    lv = _index(ab, "t3")
    pb = gb.Guarded(4, 4, name="pair_begin")
    npairs = gb.Guarded(8, 8, name="num_pairs")
    wsb = ab.lib().adl_bloom_level_candidates_workspace_bytes(0)
    ws = gb.Guarded(wsb, 256, name="workspace")
    rc = ab.lib().adl_bloom_level_candidates_device(lv._h, None, None, 0, 16, 25, pb.ptr, None, 0, npairs.ptr, ws.ptr,
                                                    wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    gb.check_all(pb, npairs, ws)
    assert pb.numpy().view(np.uint32)[0] == 0 and npairs.numpy().view(np.uint64)[0] == 0


def test_candidates_device_stream_order(dev, ab, oracle):
    """On a delayed non-default stream the selection reads the keys the
    producer wrote on that stream and its outputs are complete when the
    consumer on that stream copies them; the call itself returns while the
    delay still runs.  (The level's upload happens in its first device call,
    which is made before the case.)"""
    torch = dev
    tables, pool, want = _case(oracle, "t16", "stride16")
    lv = _index(ab, "t16")
    longest = lv.stats()[3]
    K = 600
    true_sel, decoy_sel = _select(K, len(pool), 1), _select(K, len(pool), 2)
    lists = [want[25][int(i)] for i in true_sel]
    assert lists != [want[25][int(i)] for i in decoy_sel]
    begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    flat = np.array([t for x in lists for t in x], np.uint32)
    true = np.frombuffer(b"".join(pool[int(i)] for i in true_sel), np.uint8)
    decoy = np.frombuffer(b"".join(pool[int(i)] for i in decoy_sel), np.uint8)
    warm = _run_select(torch, ab, lv, "stride16", [pool[0]], 25, longest)  # uploads the index
    assert warm[2] == len(want[25][0])
    cap = K * longest
    wsb = ab.lib().adl_bloom_level_candidates_workspace_bytes(K)
    case = so.Case()
    d_keys = case.input(true, decoy, pad=32)
    pb, pt, npairs = case.output((K + 1) * 4), case.output(cap * 4), case.output(8)
    ws = case.workspace(wsb)

    def entry(stream):
        rc = ab.lib().adl_bloom_level_candidates_device(lv._h, d_keys.data_ptr(), None, K, 16, 25, pb.data_ptr(),
                                                        pt.data_ptr(), cap, npairs.data_ptr(), ws.data_ptr(), wsb,
                                                        so.sptr(stream))
        assert rc == 0, rc

    case.run(entry)
    assert case.returned_early, "the call came back only after the delay: it waits for the stream"
    so.check(case.result(npairs), np.array([len(flat)], np.uint64), "num_pairs")
    so.check(case.result(pb), begin, "pair_begin")
    so.check(case.result(pt, 4 * len(flat)), flat, "pair_table")
    so.release_delay()


# ------------------------------------------------------------------ multi-get through a cache
def _multiget_level(oracle):
    """Five overlapping tables of var-len user keys (bits_per_key 3, 10, 44, 10, 3), the last never cached."""
    rng = np.random.default_rng(4242)
    bpks = [3, 10, 44, 10, 3]
    universe = sorted({bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)) for _ in range(6000)})
    tabs = []
    for t, bpk in enumerate(bpks):
        lo = 700 * t
        members = universe[lo:lo + 2400:2]  # every other key of its range: the rest are absent inside it
        bm = oracle.keys2block(members, bits_per_key=bpk)
        tabs.append({"members": members, "bpk": bpk, "bitmap": bm, "block": oracle.filter_block_final([bm.tobytes()], bpk),
                     "range": (inner(members[0], 9, 0), inner(members[-1], *_max_tail(t))), "oid": b"lvl-%d" % t})
    return universe, tabs


def _expected_answers(oracle, tabs, keys, begin, table, cached):
    owner = np.repeat(np.arange(len(keys)), np.diff(begin.astype(np.int64)))
    ekeys = [keys[int(i)] for i in owner]
    bms = [t["bitmap"].tobytes() for t in tabs]
    off = np.concatenate([[0], np.cumsum([len(b) for b in bms])]).astype(np.uint64)
    allbm = np.frombuffer(b"".join(bms) + bytes(16), np.uint8)
    want = np.ones(len(table), np.uint8)
    for bpk in sorted({t["bpk"] for t in tabs}):
        s = np.flatnonzero(np.array([cached[int(t)] and tabs[int(t)]["bpk"] == bpk for t in table], bool))
        if len(s):
            want[s] = oracle.probe_multi([ekeys[int(i)] for i in s], table[s], allbm, off, bits_per_key=bpk)
    return want


@pytest.mark.parametrize("K", [700, 20000], ids=["one_copy", "two_phase"])
def test_level_multiget_through_cache(dev, ab, oracle, K):
    universe, tabs = _multiget_level(oracle)
    tables = [t["range"] for t in tabs]
    oids = [t["oid"] for t in tabs]
    cache = ab.FilterCache(16 << 20, max_tables=16)
    lv = ab.LevelIndex(tables, oids=oids)
    try:
        for t in tabs[:4]:
            cache.put(t["oid"], t["block"])
        cached = [True, True, True, True, False]
        rng = np.random.default_rng(K)
        pool = [universe[int(i)] for i in rng.integers(0, len(universe), 1500)]
        pool += [_user(r[1]) for r in tables] + [_user(r[0]) for r in tables] + [b"", b"\xff" * 41]
        keys = [pool[int(i)] for i in _select(K, len(pool), 9)]
        data, offs = oracle.pack(keys)
        per_pool = {}
        for step, seq in enumerate((25, SEQ_MAX)):
            if step == 1:
                assert cache.remove(oids[2])  # evicted mid-test: answers 1 from now on
                cached[2] = False
            lists = [per_pool.setdefault((k, seq), oracle.level_candidates(tables, k, seq)) for k in keys]
            begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
            flat = np.array([t for x in lists for t in x], np.uint32)
            pb, pt, out, unc = lv.multiget(cache, data, offs, seq=seq)
            assert np.array_equal(pb, begin) and np.array_equal(pt, flat)
            want = _expected_answers(oracle, tabs, keys, begin, flat, cached)
            assert np.array_equal(out, want), int((out != want).sum())
            want_unc = int(sum(not cached[int(t)] for t in flat))
            assert unc == want_unc and unc > 0
            ref, ref_unc = cache.probe_fanout(oids, begin, flat, data, offs)
            assert out.tobytes() == ref.tobytes() and ref_unc == unc
            hit_cached = want[np.array([cached[int(t)] for t in flat], bool)]
            assert 0 < int(hit_cached.sum()) < len(hit_cached)
            # too small a capacity: ADL_ERR_WORKSPACE, the total reported, begin complete
            rc, pb2, _, _, n2, _ = lv.multiget_status(cache, data, offs, seq=seq, pair_capacity=len(flat) - 1)
            assert rc == ab.ADL_ERR_WORKSPACE and n2 == len(flat) and np.array_equal(pb2, begin)
            # ... and the table and answer buffers left as they were
            pb3 = np.zeros(K + 1, np.uint32)
            pt3 = np.full(len(flat), 0xA5A5A5A5, np.uint32)
            out3 = np.full(len(flat), 0xA5, np.uint8)
            n3, unc3 = ctypes.c_uint64(), ctypes.c_uint64()
            rc = ab.lib().adl_bloom_level_multiget(lv._h, cache._h, 0, data.ctypes.data, offs.ctypes.data, K, 0, seq,
                                                   pb3.ctypes.data, pt3.ctypes.data, out3.ctypes.data, len(flat) - 1,
                                                   ctypes.byref(n3), ctypes.byref(unc3), None)
            assert rc == ab.ADL_ERR_WORKSPACE and n3.value == len(flat) and np.array_equal(pb3, begin)
            assert (pt3 == 0xA5A5A5A5).all() and (out3 == 0xA5).all()
        # a level created without oids selects but cannot multi-get
        bare = ab.LevelIndex(tables)
        rc = bare.multiget_status(cache, data, offs)[0]
        assert rc == -1
        bare.close()
    finally:
        lv.close()
        cache.close()


def test_level_multiget_short_capacity_releases_its_pins(dev, ab, oracle):
    """adl_bloom_level_multiget returning ADL_ERR_WORKSPACE has unpinned the
    level's tables: removed right after, their arena ranges are free at once
    (a range still pinned would stay in use).  The next full-capacity call on
    the re-populated cache answers as probe_fanout does on the same lists."""
    _, tabs = _multiget_level(oracle)
    tabs = tabs[:4]
    oids = [t["oid"] for t in tabs]
    keys = [t["members"][i] for t in tabs for i in (100, 500)]  # 8 keys, each inside its table's range
    data, offs = oracle.pack(keys)
    cache = ab.FilterCache(16 << 20, max_tables=16)
    lv = ab.LevelIndex([t["range"] for t in tabs], oids=oids)
    try:
        for t in tabs:
            cache.put(t["oid"], t["block"])
        rc, _, _, _, n, _ = lv.multiget_status(cache, data, offs, pair_capacity=1)
        assert rc == ab.ADL_ERR_WORKSPACE and n >= len(keys)
        assert all(cache.remove(o) for o in oids)
        assert cache.stats() == (0, 0)
        for t in tabs:
            cache.put(t["oid"], t["block"])
        pb, pt, out, unc = lv.multiget(cache, data, offs)
        assert (np.diff(pb.astype(np.int64)) > 0).all() and len(pt) == n and unc == 0
        ref, ref_unc = cache.probe_fanout(oids, pb, pt, data, offs)
        assert out.tobytes() == ref.tobytes() and ref_unc == 0
    finally:
        lv.close()
        cache.close()


def test_level_index_binary(dev):
    """bin/level_index_test: LevelMultiGetFilter(cache, index, ...) on the host
    copy (300 keys) and on the device path (3 000 keys) equals
    LevelMultiGetFilter(cache, tables, ...) on a 12-table overlapping level and
    a 2 000-table disjoint one, at four sequence numbers."""
    exe = os.path.join(ROOT, "adlsm-tree_amd", "bin", "level_index_test")
    assert os.path.exists(exe), f"{exe} is missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if k != "ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
