"""GPU: the revision multi-get (adlsm-tree_amd/csrc/revision_index.hip, the hit
kernels of bloom_probe.hip, adl_bloom_revision_multiget in filter_cache.hip).

* adl_bloom_revision_candidates_device against oracle.level_candidates per
  level, concatenated level 0 first as global ids (tests/revisionkeys.py): begin
  and lists exact over 1 / 255 / 256 / 257 / 1000 keys, revisions of 1 level
  (byte for byte adl_bloom_level_candidates_device on that level), 2 levels, 5
  with an empty and a NULL one in the middle, 8, the 300-table level twice (a
  key with 600 candidates) and a level of 514 boundaries beside one of 50, at
  seq 24 / 25 / 26, through var-len offsets, stride 16, stride 24 and an
  unaligned base; a pair capacity smaller than needed, in guard bands;
* adl_bloom_probe_fanout_hits_device against adl_bloom_probe_fanout_device plus
  a numpy filter on the same pair arrays: every pair hits, none does, only the
  last pair of a key, keys without pairs, filter ids >= num_filters, an empty
  filter, a key of 600 pairs whose hits are scattered over the compaction
  rounds, key counts around 256, a short hit capacity in guard bands, no keys,
  no pairs;
* stream order of both entry points behind a delay on a non-default stream;
* adl_bloom_revision_multiget over three levels through a cache of blocks of
  bits_per_key 3, 10 and 44, one table never cached and one removed mid-test:
  the hits against the oracle and against adl_bloom_level_multiget per level,
  the uncached count, ADL_ERR_WORKSPACE for a short hit and a short pair
  capacity, filter 1 on one-filter blocks;
* bin/revision_test: the C++ overload on both sides of its threshold, and
  --race: eight threads racing the first device call on one revision."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import guardband as gb
import revisionkeys as rk
import streamorder as so
from test_gpu_level_index import _device_keys, _expected_answers, _max_tail, _select, _user, inner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 255, 256, 257, 1000)
SHAPES = tuple(rk.REVISIONS)
VIEWS = ("var", "stride16", "stride24", "unaligned")
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


_levels = {}
_revs = {}


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for r in _revs.values():
        r.close()
    for lv in _levels.values():
        lv.close()
    _revs.clear()
    _levels.clear()


def _level(ab, name):
    if name is None:
        return None
    if name not in _levels:
        _levels[name] = ab.LevelIndex(rk.tables(name))
    return _levels[name]


def _rev(ab, shape):
    if shape not in _revs:
        _revs[shape] = ab.Revision([_level(ab, n) for n in rk.REVISIONS[shape]])
    return _revs[shape]


def _run_candidates(torch, ab, rev, view, keys, seq, cap):
    """One adl_bloom_revision_candidates_device call into guarded buffers: (begin, table[:cap], num_pairs)."""
    K = len(keys)
    kp, op, stride, keep = _device_keys(torch, view, keys)
    wsb = ab.lib().adl_bloom_revision_candidates_workspace_bytes(rev._h, K)
    pb = gb.Guarded((K + 1) * 4, 4, name="pair_begin")
    pt = gb.Guarded(cap * 4, 4, name="pair_table")
    npairs = gb.Guarded(8, 8, name="num_pairs")
    ws = gb.Guarded(wsb, 256, name="workspace")
    rc = ab.lib().adl_bloom_revision_candidates_device(rev._h, kp, op, K, stride, seq, pb.ptr, pt.ptr, cap, npairs.ptr,
                                                       ws.ptr, wsb, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    gb.check_all(pb, pt, npairs, ws)
    del keep
    return pb.numpy().view(np.uint32), pt.numpy().view(np.uint32), int(npairs.numpy().view(np.uint64)[0])


def _check_candidates(torch, ab, oracle, shape, view, K, seed):
    names = rk.REVISIONS[shape]
    stride = {"stride16": 16, "stride24": 24}.get(view)
    pool = rk.pool(names, stride)
    rev = _rev(ab, shape)
    longest = rev.stats()[2]
    keys = [pool[int(i)] for i in _select(K, len(pool), seed)]
    seen = 0
    for seq in rk.SEQS:
        lists = rk.revision_lists(oracle, names, keys, seq)
        begin, flat = rk.csr(lists)
        assert max(len(x) for x in lists) <= longest
        got_b, got_t, got_n = _run_candidates(torch, ab, rev, view, keys, seq, max(len(flat), 1))
        assert got_n == len(flat), (seq, got_n, len(flat))
        assert np.array_equal(got_b, begin), (seq, int(np.flatnonzero(got_b != begin)[0]))
        for i, x in enumerate(lists):
            assert list(got_t[begin[i]:begin[i + 1]]) == x, (seq, i, keys[i])
        seen += len(flat)
    return keys, seen


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_candidates_device_vs_oracle(dev, ab, oracle, shape, K):
    keys, seen = _check_candidates(dev, ab, oracle, shape, "var", K, SHAPES.index(shape) * 10 + KS.index(K))
    if K >= 255:
        assert seen > 0
        names = rk.REVISIONS[shape]
        most = max(len(x) for x in rk.revision_lists(oracle, names, keys, 26))
        if shape == "twice300":
            assert most == 600  # one key with more candidates than two rounds of a workgroup
        if shape == "wide":
            assert _level(ab, "t257").stats()[0] == 2 * 514 + 1 and _level(ab, "t16").stats()[0] < 2 * 512


@pytest.mark.parametrize("view", VIEWS[1:])
@pytest.mark.parametrize("shape,K", [("five", 1000), ("wide", 257)])
def test_candidates_device_key_views(dev, ab, oracle, shape, K, view):
    _, seen = _check_candidates(dev, ab, oracle, shape, view, K, 500 + VIEWS.index(view))
    assert seen > 0


@pytest.mark.parametrize("K", KS)
def test_one_level_equals_the_level_call(dev, ab, K):
    """A revision of one level gives adl_bloom_level_candidates_device's bytes."""
    torch = dev
    names = rk.REVISIONS["one"]
    pool = rk.pool(names)
    rev, lv = _rev(ab, "one"), _level(ab, names[0])
    keys = [pool[int(i)] for i in _select(K, len(pool), 31 + K)]
    cap = K * lv.stats()[3]
    for seq in rk.SEQS:
        got_b, got_t, got_n = _run_candidates(torch, ab, rev, "var", keys, seq, cap)
        kp, op, stride, keep = _device_keys(torch, "var", keys)
        wsb = ab.lib().adl_bloom_level_candidates_workspace_bytes(K)
        pb, pt, n, ws = gb.Guarded((K + 1) * 4, 4), gb.Guarded(cap * 4, 4), gb.Guarded(8, 8), gb.Guarded(wsb, 256)
        assert ab.lib().adl_bloom_level_candidates_device(lv._h, kp, op, K, stride, seq, pb.ptr, pt.ptr, cap, n.ptr,
                                                          ws.ptr, wsb, None) == 0
        torch.cuda.synchronize()
        total = int(n.numpy().view(np.uint64)[0])
        assert got_n == total and got_b.tobytes() == pb.numpy().tobytes()
        assert got_t[:total].tobytes() == pt.numpy().view(np.uint32)[:total].tobytes()


def test_pair_capacity_smaller_than_needed(dev, ab, oracle):
    """begin complete, *d_num_pairs exact, the first `cap` entries right and
    nothing written past them (the table buffer is exactly cap entries inside
    guard bands)."""
    torch = dev
    for shape, K in (("five", 1000), ("twice300", 257)):
        names = rk.REVISIONS[shape]
        pool = rk.pool(names)
        keys = [pool[int(i)] for i in _select(K, len(pool), 77)]
        begin, flat = rk.csr(rk.revision_lists(oracle, names, keys, 25))
        total = len(flat)
        for cap in (total // 2, 1, total - 1):
            got_b, got_t, got_n = _run_candidates(torch, ab, _rev(ab, shape), "var", keys, 25, cap)
            assert got_n == total and np.array_equal(got_b, begin)
            assert np.array_equal(got_t, flat[:cap]), cap


def test_zero_keys_and_empty_revision(dev, ab):
    torch = dev
    rev = _rev(ab, "two")
    pb = gb.Guarded(4, 4, name="pair_begin")
    npairs = gb.Guarded(8, 8, name="num_pairs")
    wsb = ab.lib().adl_bloom_revision_candidates_workspace_bytes(rev._h, 0)
    ws = gb.Guarded(wsb, 256, name="workspace")
    assert ab.lib().adl_bloom_revision_candidates_device(rev._h, None, None, 0, 16, 25, pb.ptr, None, 0, npairs.ptr,
                                                         ws.ptr, wsb, None) == 0
    torch.cuda.synchronize()
    gb.check_all(pb, npairs, ws)
    assert pb.numpy().view(np.uint32)[0] == 0 and npairs.numpy().view(np.uint64)[0] == 0
    # every level empty or missing: no key has a candidate
    empty = ab.Revision([None, ab.LevelIndex([]), None])
    try:
        keys = [b"ab", b"", b"\xff" * 20]
        got_b, _, got_n = _run_candidates(torch, ab, empty, "var", keys, 25, 1)
        assert got_n == 0 and not got_b.any()
    finally:
        empty.close()


def test_candidates_device_torch_wrapper(dev, ab, oracle):
    torch = dev
    names = rk.REVISIONS["five"]
    pool = rk.pool(names, 16)
    keys = pool[:200]
    begin, flat = rk.csr(rk.revision_lists(oracle, names, keys, 25))
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 16).copy()).cuda()
    rev = _rev(ab, "five")
    pb, pt, n = rev.candidates_device(d_keys, seq=25)
    torch.cuda.synchronize()
    assert int(n.item()) == len(flat) and pt.numel() == len(keys) * rev.stats()[2]
    assert np.array_equal(pb.cpu().numpy().view(np.uint32), begin)
    assert np.array_equal(pt.cpu().numpy().view(np.uint32)[:len(flat)], flat)


# ------------------------------------------------------------------ probe_fanout_hits
def _sets(oracle, bpk, stride=None):
    """Two disjoint key sets, absent keys, and the filters [A, B, empty, A + B].  stride: None for var-len keys
    of 1 to 39 bytes, else keys of that size."""
    rng = np.random.default_rng(bpk)
    keys = sorted({rng.integers(0, 256, stride or int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
                   for _ in range(900)})
    assert len(keys) >= 890
    a, b, absent = keys[0:300], keys[300:600], keys[600:900]
    bms = [oracle.keys2block(a, bits_per_key=bpk).tobytes(), oracle.keys2block(b, bits_per_key=bpk).tobytes(), b"",
           oracle.keys2block(a + b, bits_per_key=bpk).tobytes()]
    off = np.concatenate([[0], np.cumsum([len(x) for x in bms])]).astype(np.uint64)
    return a, b, absent, np.frombuffer(b"".join(bms) + bytes(16), np.uint8), off


def _check_hits(torch, ab, keys, pb, pf, bm, off, bpk, cap=None):
    """adl_bloom_probe_fanout_hits_device into guarded buffers against probe_fanout's answers on the same
    arrays, filtered with numpy.  cap: the hit capacity (default: exactly the hits).  -> (hits, pairs)."""
    K, P = len(keys), len(pf)
    offs = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys) + bytes(16), np.uint8).copy()).cuda()
    d_offs = torch.from_numpy(offs).cuda()
    d_pb = torch.from_numpy(pb.astype(np.uint32).view(np.int32).copy()).cuda()
    d_pf = torch.from_numpy(np.concatenate([pf.astype(np.uint32), np.zeros(1, np.uint32)]).view(np.int32)).cuda()[:P]
    d_bm = torch.from_numpy(bm.copy()).cuda()
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    ans = ab.probe_fanout(d_keys, d_pb, d_pf, d_bm, d_off, offsets=d_offs, bits_per_key=bpk)
    torch.cuda.synchronize()
    ans = ans.cpu().numpy().astype(bool) if P else np.zeros(0, bool)
    owner = np.repeat(np.arange(K), np.diff(pb.astype(np.int64)))
    want_t = pf.astype(np.uint32)[ans]
    want_b = np.concatenate([[0], np.cumsum(np.bincount(owner[ans], minlength=K))]).astype(np.uint32)
    cap = len(want_t) if cap is None else cap
    wsb = ab.lib().adl_bloom_probe_fanout_hits_workspace_bytes(K, P)
    hb = gb.Guarded((K + 1) * 4, 4, name="hit_begin")
    hf = gb.Guarded(cap * 4, 4, name="hit_filter")
    nh = gb.Guarded(8, 8, name="num_hits")
    ws = gb.Guarded(wsb, 256, name="workspace")
    rc = ab.lib().adl_bloom_probe_fanout_hits_device(d_keys.data_ptr(), d_offs.data_ptr(), K, 0, d_pb.data_ptr(),
                                                     d_pf.data_ptr(), P, len(off) - 1, d_bm.data_ptr(),
                                                     d_off.data_ptr(), None, bpk, hb.ptr, hf.ptr, cap, nh.ptr, ws.ptr,
                                                     wsb, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    gb.check_all(hb, hf, nh, ws)
    assert int(nh.numpy().view(np.uint64)[0]) == len(want_t)
    got_b = hb.numpy().view(np.uint32)
    assert np.array_equal(got_b, want_b), int(np.flatnonzero(got_b != want_b)[0])
    m = min(cap, len(want_t))
    assert np.array_equal(hf.numpy().view(np.uint32)[:m], want_t[:m])
    return len(want_t), P


def _csr_counts(cnt):
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)


@pytest.mark.parametrize("K", KS)
def test_hits_every_pair_and_no_pair(dev, ab, oracle, K):
    torch = dev
    rng = np.random.default_rng(K)
    # every pair hits: the keys were inserted into all their filters (bits_per_key 10)
    a, b, absent, bm, off = _sets(oracle, 10)
    keys = [a[int(i)] for i in rng.integers(0, len(a), K)]
    pb = _csr_counts(rng.integers(0, 6, K))
    pf = rng.choice([0, 3], int(pb[-1]))
    hits, pairs = _check_hits(torch, ab, keys, pb, pf, bm, off, 10)
    assert hits == pairs and (pairs > 0 or K == 1)
    # no pair hits: absent keys, and bits_per_key 44 (30 probes) leaves no false positive
    a, b, absent, bm, off = _sets(oracle, 44)
    keys = [absent[int(i)] for i in rng.integers(0, len(absent), K)]
    pf = rng.choice([0, 1, 3], int(pb[-1]))
    hits, pairs = _check_hits(torch, ab, keys, pb, pf, bm, off, 44)
    assert hits == 0


@pytest.mark.parametrize("K", KS)
def test_hits_mixed_situations(dev, ab, oracle, K):
    """Only the last pair of a key hits; keys without pairs; filter ids >=
    num_filters; the empty filter; a key of 600 pairs, every third a hit, at
    the edge of a key block; false positives at bits_per_key 3."""
    torch = dev
    rng = np.random.default_rng(100 + K)
    a, b, absent, bm, off = _sets(oracle, 44)
    keys, lists = [], []
    for i in range(K):
        kind = i % 5
        k = a[int(rng.integers(0, len(a)))]
        if kind == 0:
            lists.append([1] * int(rng.integers(1, 5)) + [0])     # filter B misses, the last pair (A) hits
        elif kind == 1:
            lists.append([])                                       # no pairs
        elif kind == 2:
            lists.append([4, 0, 9, 2, 3])                          # ids >= num_filters and the empty filter answer 0
        elif kind == 3:
            k = absent[int(rng.integers(0, len(absent)))]
            lists.append([0, 1, 3])                                # nothing hits
        else:
            lists.append([int(x) for x in rng.choice([0, 1], int(rng.integers(0, 8)))])
        keys.append(k)
    hot = min(255, K - 1)
    keys[hot] = a[7]
    lists[hot] = [0 if p % 3 == 0 else 1 for p in range(600)]       # 200 hits scattered over three rounds
    pb = _csr_counts([len(x) for x in lists])
    pf = np.array([f for x in lists for f in x], np.uint32)
    hits, pairs = _check_hits(torch, ab, keys, pb, pf, bm, off, 44)
    assert 200 <= hits < pairs
    # bits_per_key 3: two probes, false positives among the misses
    a3, b3, absent3, bm3, off3 = _sets(oracle, 3)
    keys3 = [(a3 + absent3)[int(i)] for i in rng.integers(0, 600, K)]
    hits3, _ = _check_hits(torch, ab, keys3, pb, pf, bm3, off3, 3)
    if K >= 255:
        assert 0 < hits3 < pairs


def test_hits_short_capacity_and_nothing_to_do(dev, ab, oracle):
    torch = dev
    rng = np.random.default_rng(5)
    a, b, absent, bm, off = _sets(oracle, 10)
    K = 700
    keys = [a[int(i)] for i in rng.integers(0, len(a), K)]
    pb = _csr_counts(rng.integers(0, 6, K))
    pf = rng.choice([0, 1, 3], int(pb[-1]))
    full, pairs = _check_hits(torch, ab, keys, pb, pf, bm, off, 10)
    assert 300 < full < pairs
    for cap in (full // 2, 1, full - 1, 0):
        assert _check_hits(torch, ab, keys, pb, pf, bm, off, 10, cap=cap)[0] == full
    # no pairs at all; no keys at all
    assert _check_hits(torch, ab, keys, np.zeros(K + 1, np.uint32), np.zeros(0, np.uint32), bm, off, 10) == (0, 0)
    assert _check_hits(torch, ab, [], np.zeros(1, np.uint32), np.zeros(0, np.uint32), bm, off, 10) == (0, 0)


def test_hits_torch_wrapper(dev, ab, oracle):
    torch = dev
    rng = np.random.default_rng(6)
    a, b, absent, bm, off = _sets(oracle, 10, 16)
    K = 300
    keys = np.frombuffer(b"".join(a[:150] + absent[:150]), np.uint8).reshape(K, 16)
    pb = _csr_counts(rng.integers(0, 4, K))
    pf = rng.choice([0, 1, 2, 3], int(pb[-1])).astype(np.uint32)
    d = [torch.from_numpy(x).cuda() for x in (keys.copy(), pb.view(np.int32), pf.view(np.int32), bm.copy(),
                                              off.view(np.int64))]
    ans = ab.probe_fanout(*d, bits_per_key=10).cpu().numpy().astype(bool)
    hb, hf, nh = ab.probe_fanout_hits(*d, bits_per_key=10)
    torch.cuda.synchronize()
    assert 0 < int(ans.sum()) < len(pf)
    assert int(nh.item()) == int(ans.sum()) and hf.numel() == len(pf)
    assert np.array_equal(hf.cpu().numpy().view(np.uint32)[:int(ans.sum())], pf[ans])
    assert hb.cpu().numpy().view(np.uint32)[-1] == ans.sum()


# ------------------------------------------------------------------ stream order
def test_candidates_device_stream_order(dev, ab, oracle):
    """On a delayed non-default stream the selection reads the keys the
    producer wrote on that stream, its outputs are complete when the consumer
    copies them, and the call returns while the delay still runs.  (The device
    copies are made by the first device call, before the case.)"""
    torch = dev
    names = rk.REVISIONS["two"]
    pool = rk.pool(names, 16)
    rev = _rev(ab, "two")
    longest = rev.stats()[2]
    K = 600
    true_sel, decoy_sel = _select(K, len(pool), 1), _select(K, len(pool), 2)
    lists = rk.revision_lists(oracle, names, [pool[int(i)] for i in true_sel], 25)
    assert lists != rk.revision_lists(oracle, names, [pool[int(i)] for i in decoy_sel], 25)
    begin, flat = rk.csr(lists)
    true = np.frombuffer(b"".join(pool[int(i)] for i in true_sel), np.uint8)
    decoy = np.frombuffer(b"".join(pool[int(i)] for i in decoy_sel), np.uint8)
    _run_candidates(torch, ab, rev, "stride16", [pool[0]], 25, longest)  # uploads the revision and its levels
    cap = K * longest
    wsb = ab.lib().adl_bloom_revision_candidates_workspace_bytes(rev._h, K)
    case = so.Case()
    d_keys = case.input(true, decoy, pad=32)
    pb, pt, npairs = case.output((K + 1) * 4), case.output(cap * 4), case.output(8)
    ws = case.workspace(wsb)

    def entry(stream):
        rc = ab.lib().adl_bloom_revision_candidates_device(rev._h, d_keys.data_ptr(), None, K, 16, 25, pb.data_ptr(),
                                                           pt.data_ptr(), cap, npairs.data_ptr(), ws.data_ptr(), wsb,
                                                           so.sptr(stream))
        assert rc == 0, rc

    case.run(entry)
    assert case.returned_early, "the call came back only after the delay: it waits for the stream"
    so.check(case.result(npairs), np.array([len(flat)], np.uint64), "num_pairs")
    so.check(case.result(pb), begin, "pair_begin")
    so.check(case.result(pt, 4 * len(flat)), flat, "pair_table")
    so.release_delay()


def test_probe_fanout_hits_stream_order(dev, ab, oracle):
    torch = dev
    rng = np.random.default_rng(8)
    a, b, absent, bm, off = _sets(oracle, 44, 16)
    K = 600
    pb = _csr_counts(rng.integers(1, 5, K))
    pf = rng.choice([0, 1, 3], int(pb[-1])).astype(np.uint32)
    owner = np.repeat(np.arange(K), np.diff(pb.astype(np.int64)))

    def batch(seed):
        r = np.random.default_rng(seed)
        return [(a + b)[int(i)] for i in r.integers(0, 600, K)]

    keys, decoys = batch(1), batch(2)
    ans = oracle.probe_multi([keys[int(i)] for i in owner], pf, bm, off, bits_per_key=44).astype(bool)
    want_t = pf[ans]
    want_b = np.concatenate([[0], np.cumsum(np.bincount(owner[ans], minlength=K))]).astype(np.uint32)
    assert 0 < len(want_t) < len(pf)
    wsb = ab.lib().adl_bloom_probe_fanout_hits_workspace_bytes(K, len(pf))
    case = so.Case()
    d_keys = case.input(np.frombuffer(b"".join(keys), np.uint8), np.frombuffer(b"".join(decoys), np.uint8), pad=32)
    d_pb, d_pf, d_bm, d_off = case.const(pb), case.const(pf), case.const(bm), case.const(off)
    hb, hf, nh = case.output((K + 1) * 4), case.output(len(pf) * 4), case.output(8)
    ws = case.workspace(wsb)

    def entry(stream):
        rc = ab.lib().adl_bloom_probe_fanout_hits_device(d_keys.data_ptr(), None, K, 16, d_pb.data_ptr(),
                                                         d_pf.data_ptr(), len(pf), len(off) - 1, d_bm.data_ptr(),
                                                         d_off.data_ptr(), None, 44, hb.data_ptr(), hf.data_ptr(),
                                                         len(pf), nh.data_ptr(), ws.data_ptr(), wsb, so.sptr(stream))
        assert rc == 0, rc

    case.run(entry)
    assert case.returned_early, "the call came back only after the delay: it waits for the stream"
    so.check(case.result(nh), np.array([len(want_t)], np.uint64), "num_hits")
    so.check(case.result(hb), want_b, "hit_begin")
    so.check(case.result(hf, 4 * len(want_t)), want_t, "hit_filter")
    so.release_delay()


# ------------------------------------------------------------------ multi-get through a cache
def _multiget_revision(oracle):
    """Three levels of overlapping tables of var-len user keys: bits_per_key (3, 10), (44, 10) and (3); the last
    table is never cached.  -> (universe, tables in global order, the levels as lists of global ids)."""
    rng = np.random.default_rng(4243)
    bpks = [3, 10, 44, 10, 3]
    universe = sorted({bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)) for _ in range(6000)})
    tabs = []
    for t, bpk in enumerate(bpks):
        lo = 700 * t
        members = universe[lo:lo + 2400:2]  # every other key of its range: the rest are absent inside it
        bm = oracle.keys2block(members, bits_per_key=bpk)
        tabs.append({"members": members, "bpk": bpk, "bitmap": bm, "block": oracle.filter_block_final([bm.tobytes()], bpk),
                     "range": (inner(members[0], 9, 0), inner(members[-1], *_max_tail(t))), "oid": b"rev-%d" % t})
    return universe, tabs, [[0, 1], [2, 3], [4]]


def _hits_of(begin, flat, answers):
    """The pairs answered 1, per key: (hit_begin, hit_table)."""
    owner = np.repeat(np.arange(len(begin) - 1), np.diff(begin.astype(np.int64)))
    keep = answers.astype(bool)
    hb = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=len(begin) - 1))]).astype(np.uint32)
    return hb, flat[keep]


@pytest.mark.parametrize("K", [700, 20000], ids=["one_copy", "two_phase"])
def test_revision_multiget_through_cache(dev, ab, oracle, K):
    universe, tabs, split = _multiget_revision(oracle)
    cache = ab.FilterCache(16 << 20, max_tables=16)
    levels = [ab.LevelIndex([tabs[t]["range"] for t in ids], oids=[tabs[t]["oid"] for t in ids]) for ids in split]
    rev = ab.Revision(levels)
    base = [ids[0] for ids in split]
    try:
        assert list(rev.stats()[1]) == [0, 2, 4, 5]
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
            want_unc = int(sum(not cached[int(t)] for t in want_t))
            hb, ht, unc = rev.multiget(cache, data, offs, seq=seq)
            assert np.array_equal(hb, want_b) and np.array_equal(ht, want_t)
            assert unc == want_unc and unc > 0
            assert unc == int(sum(not cached[int(t)] for t in flat))  # every pair of an uncached table is a hit
            hit_cached = int(sum(cached[int(t)] for t in want_t))
            assert 0 < hit_cached < int(sum(cached[int(t)] for t in flat))
            # ... and equal to the level multi-gets, one per level, filtered on the host
            per = [lv.multiget(cache, data, offs, seq=seq) for lv in levels]
            rows = []
            for i in range(K):
                row = []
                for l, (pb, pt, out, _) in enumerate(per):
                    s = slice(int(pb[i]), int(pb[i + 1]))
                    row += [base[l] + int(t) for t, m in zip(pt[s], out[s]) if m]
                rows.append(row)
            ref_b, ref_t = rk.csr(rows)
            assert np.array_equal(hb, ref_b) and np.array_equal(ht, ref_t)
            assert unc == sum(int(p[3]) for p in per)
            # a short hit capacity: ADL_ERR_WORKSPACE, both totals reported, hit_begin complete
            rc, hb2, _, nh2, np2, _ = rev.multiget_status(cache, data, offs, seq=seq, hit_capacity=len(want_t) - 1)
            assert rc == ab.ADL_ERR_WORKSPACE and nh2 == len(want_t) and np2 == len(flat)
            assert np.array_equal(hb2, want_b)
            # a short pair capacity: ADL_ERR_WORKSPACE, the pair total reported, nothing else written
            hb3 = np.full(K + 1, 0xA5A5A5A5, np.uint32)
            ht3 = np.full(len(flat), 0xA5A5A5A5, np.uint32)
            nh3, np3, unc3 = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            rc = ab.lib().adl_bloom_revision_multiget(rev._h, cache._h, 0, data.ctypes.data, offs.ctypes.data, K, 0,
                                                      seq, hb3.ctypes.data, ht3.ctypes.data, len(flat),
                                                      ctypes.byref(nh3), len(flat) - 1, ctypes.byref(np3),
                                                      ctypes.byref(unc3), None)
            assert rc == ab.ADL_ERR_WORKSPACE and np3.value == len(flat)
            assert (hb3 == 0xA5A5A5A5).all() and (ht3 == 0xA5A5A5A5).all()
            # an exact pair capacity is enough
            rc, hb4, ht4, _, np4, _ = rev.multiget_status(cache, data, offs, seq=seq, pair_capacity=len(flat))
            assert rc == 0 and np4 == len(flat) and np.array_equal(hb4, want_b) and np.array_equal(ht4, want_t)
            # filter 1 on blocks of one filter: no hit from a cached table
            hb5, ht5, unc5 = rev.multiget(cache, data, offs, seq=seq, filter=1)
            assert unc5 == want_unc == len(ht5) and not any(cached[int(t)] for t in ht5)
        # no keys: nothing to do
        rc, hb6, ht6, nh6, np6, _ = rev.multiget_status(cache, np.zeros((0, 16), np.uint8))
        assert rc == 0 and nh6 == 0 and np6 == 0 and list(hb6) == [0]
        # a level created without oids selects but cannot multi-get
        bare_lv = ab.LevelIndex([tabs[t]["range"] for t in split[0]])
        bare = ab.Revision([bare_lv])
        assert bare.multiget_status(cache, data, offs)[0] == -1
        bare.close()
        bare_lv.close()
    finally:
        rev.close()
        for lv in levels:
            lv.close()
        cache.close()


def test_revision_multiget_short_capacities_release_their_pins(dev, ab, oracle):
    """adl_bloom_revision_multiget returning ADL_ERR_WORKSPACE, for too few hits
    and for too few pairs, has unpinned every level's tables: removed right
    after, their arena ranges are free at once.  The next full-capacity call on
    the re-populated cache keeps the pairs probe_fanout answers 1 on the same
    lists."""
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
        rc, _, _, nh, npairs, _ = rev.multiget_status(cache, data, offs, hit_capacity=1)
        assert rc == ab.ADL_ERR_WORKSPACE and npairs >= nh >= len(keys)
        rc, _, _, _, np2, _ = rev.multiget_status(cache, data, offs, pair_capacity=1)
        assert rc == ab.ADL_ERR_WORKSPACE and np2 == npairs
        assert all(cache.remove(o) for o in oids)
        assert cache.stats() == (0, 0)
        for t in tabs:
            cache.put(t["oid"], t["block"])
        hb, ht, unc = rev.multiget(cache, data, offs)
        per = [lv.multiget(cache, data, offs) for lv in levels]
        begin, flat = rk.csr([[ids[0] + int(t) for ids, (pb, pt, _, _) in zip(split, per)
                               for t in pt[int(pb[i]):int(pb[i + 1])]] for i in range(len(keys))])
        assert (np.diff(begin.astype(np.int64)) > 0).all() and len(flat) == npairs
        ref, ref_unc = cache.probe_fanout(oids, begin, flat, data, offs)
        want_b, want_t = _hits_of(begin, flat, ref)
        assert np.array_equal(hb, want_b) and np.array_equal(ht, want_t) and len(ht) == nh
        assert unc == ref_unc == 0
    finally:
        rev.close()
        for lv in levels:
            lv.close()
        cache.close()


def test_revision_binary(dev):
    """bin/revision_test: RevisionMultiGetFilter on the per-level loop (300
    keys) and on the single device call (3 000 keys) equals one
    LevelMultiGetFilter per level with the hits kept, over five levels with an
    empty and a missing one, at four sequence numbers."""
    exe = os.path.join(ROOT, "adlsm-tree_amd", "bin", "revision_test")
    assert os.path.exists(exe), f"{exe} is missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items()
           if k not in ("ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS", "ADL_BLOOM_REVISION_DEVICE_MIN_KEYS")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout


def test_revision_binary_race(dev):
    """bin/revision_test --race: eight threads whose first call on one shared
    revision, over levels that were never asked either, is the 3 000-key single
    device call (the handles' call_once and the uploads of the revision's and
    the levels' device copies race); every result equals the per-level loop's."""
    exe = os.path.join(ROOT, "adlsm-tree_amd", "bin", "revision_test")
    assert os.path.exists(exe), f"{exe} is missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items()
           if k not in ("ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS", "ADL_BLOOM_REVISION_DEVICE_MIN_KEYS")}
    r = subprocess.run([exe, "--race"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
