"""GPU: the resident level index (adlsm-tree_amd/csrc/level_index.hip) at the
sizes tests/test_gpu_level_index.py stops short of.  Everything is compared
exactly with oracle.level_candidates / oracle.probe_multi.

1. scan runs: 65 536 to 200 001 keys, so level_scan_kernel's threads own 1, 2,
   3 and 4 workgroup totals each, with clipped and empty trailing runs;
2. a pair total just below 2^32 (the last entries written at w = 2^32 - 1 - x);
3. a total at and above 2^32 (*d_num_pairs a u64, ADL_ERR_TOO_LARGE);
4. key bytes past 2^32 at stride 320, and var-len offsets past 2^32;
5. lists of 1 000 candidates (a workgroup total above 200 000);
6. a level without tables and one whose tables all have max < min;
7. eight Python threads racing the first device call on one level;
8. the same race through the C++ LevelIndex (bin/level_index_test --race).

Large batches are drawn from a pool of at most 100 distinct keys through an
index array that lives on the device; the oracle is asked once per pool key
and sequence number, and `device_compare` checks pair_begin and pair_table
where they are, a chunk of keys at a time (only counts and first indices come
back).  Each case prints the path it reached ("reached: ..." lines, pytest -s).
"""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import guardband as gb
from test_gpu_level_index import (P40, ROOT, SEQS, _expected_answers, _level, _max_tail, _multiget_level, _pool,
                                  _select, _special_users, _user, ab, dev, inner)  # noqa: F401 (ab, dev: fixtures)

pytestmark = pytest.mark.gpu

KBLOCK = 256  # keys per workgroup, and threads of the one scan workgroup
# per = 1, 2, 2, 2, 3, 4.  65 792 = 257 full workgroups (65 537: the 257th holds one key); 65 793 adds the
# 258th, so that thread 128's run of two is full and 129.. are empty
SCAN_KS = (65536, 65537, 65792, 65793, 131073, 200001)
POOL_MAX = 100
GIB = 1 << 30


@pytest.fixture(scope="module", autouse=True)
def _peak(dev):
    dev.cuda.reset_peak_memory_stats()
    yield
    print(f"\nreached: peak of torch's device allocations over this file: "
          f"{dev.cuda.max_memory_allocated() / GIB:.2f} GiB")


# ------------------------------------------------------------------ levels
def _level320():
    """t16 and two more tables whose boundary user keys are 320 bytes long: no
    boundary of t16 is, so a stride-320 key could never equal one."""
    a, b, c = (P40 + bytes([x]) * 280 for x in (0x11, 0x7f, 0x80))
    return _level("t16") + [(inner(a, 3, 0), inner(b, *_max_tail(1))), (inner(b, 5, 1), inner(c, *_max_tail(2)))]


def _nested(T=1000):
    """T nested tables: the mins ascend, the maxes descend, so every table
    covers the middle (one region of T candidates)."""
    return [(inner(b"n%04d" % i, 9, 0), inner(b"x%04d" % (T - 1 - i), *_max_tail(i))) for i in range(T)]


def _tables(name):
    if name == "t16+320":
        return _level320()
    if name == "nested":
        return _nested()
    if name == "none":
        return []
    if name == "inverted":  # 8 tables, every max user key before its min: boundaries, but no list
        return [(inner(b"m%02d" % (2 * i + 1), 9, 0), inner(b"m%02d" % (2 * i), *_max_tail(i))) for i in range(8)]
    return _level(name)


_levels = {}


@pytest.fixture(scope="module", autouse=True)
def _close_levels():
    yield
    for lv in _levels.values():
        lv.close()
    _levels.clear()


def _index(ab, name, oids=False):
    key = (name, oids)
    if key not in _levels:
        tables = _tables(name)
        _levels[key] = ab.LevelIndex(tables, oids=[b"%s-%d" % (name.encode(), t) for t in range(len(tables))]
                                     if oids else None)
    return _levels[key]


# ------------------------------------------------------------------ pools
def _boundaries(tables):
    return sorted({_user(t[0]) for t in tables} | {_user(t[1]) for t in tables})


def _is_successor(k, users):
    """k is a boundary followed by zero bytes and no boundary itself: boundary +
    "\\0", or at a fixed stride a shorter boundary zero padded.  Its 16-byte
    prefix ties with the boundary's when that is shorter than 16 bytes."""
    return k.endswith(b"\0") and k not in users and any(k[:n] in users for n in range(len(k)) if not any(k[n:]))


def _small_pool(tables, stride):
    """At most POOL_MAX keys of test_gpu_level_index._pool(tables, stride): the
    boundaries it holds (the tables' max user keys first), their successors
    (_is_successor), the fixed edge keys, and an even sample of the rest."""
    full = _pool(tables, stride)
    users = set(_boundaries(tables))
    maxes = {_user(t[1]) for t in tables}
    if stride is not None:  # every boundary of exactly the stride (only some are in `full`)
        full = sorted(set(full) | {u for u in users if len(u) == stride})
    on_max = [k for k in full if k in maxes][:16]
    on_b = [k for k in full if k in users and k not in maxes][:16]
    succ = [k for k in full if _is_successor(k, users)][:12]
    edge = [k for k in full if k in (b"", b"ab", b"ab\0", b"\x65", b"\xff\xff\xff", bytes(300), b"\xff" * 300, P40,
                                     P40[:16], P40[:17])]
    keep = set(on_max + on_b + succ + edge)
    rest = [k for k in full if k not in keep]
    room = POOL_MAX - len(keep)
    keep |= {rest[(i * len(rest)) // room] for i in range(room)} if len(rest) > room else set(rest)
    return sorted(keep)


def _check_small_pool(tables, pool, want, stride):
    """The kinds of key test_gpu_level_index._check_pool asks for are all in the (small) pool."""
    assert 0 < len(pool) <= POOL_MAX and len(set(pool)) == len(pool)
    users = set(_boundaries(tables))
    assert any(k in users for k in pool), "no key on a boundary"
    assert any(_is_successor(k, users) for k in pool), "no boundary + \\0"
    assert any(not want[25][i] for i in range(len(pool))), "no key without candidates"
    assert any(want[24][i] != want[26][i] for i in range(len(pool))), "no list that depends on seq"
    assert len({len(x) for x in want[25]}) >= 3
    if stride is None:
        assert b"" in pool and b"ab" in pool and b"ab\0" in pool
        assert {len(k) for k in pool} >= {0, 16, 17, 300}
    sp = _special_users()
    assert sorted(sp, key=lambda k: [b - 256 if b >= 128 else b for b in k]) != sp


_cases = {}


def _case(oracle, level, stride, pool=None, check=True):
    """{tables, pool, want: {seq: per-pool-key oracle list}} once per (level, stride)."""
    key = (level, stride)
    if key not in _cases:
        tables = _tables(level)
        pool = _small_pool(tables, stride) if pool is None else pool
        want = {seq: [oracle.level_candidates(tables, k, seq) for k in pool] for seq in SEQS}
        if check:
            _check_small_pool(tables, pool, want, stride)
        _cases[key] = {"tables": tables, "pool": pool, "want": want, "dev": {}}
    return _cases[key]


def _expect(torch, case, seq):
    """The oracle's lists on the device: (len_of int64[pool], lists int32[pool, longest], padded with -1)."""
    if seq not in case["dev"]:
        lists = case["want"][seq]
        longest = max(1, max(len(x) for x in lists))
        m = np.full((len(lists), longest), -1, np.int32)
        for i, x in enumerate(lists):
            m[i, :len(x)] = x
        case["dev"][seq] = (torch.tensor([len(x) for x in lists], dtype=torch.int64).cuda(),
                            torch.from_numpy(m).cuda())
    return case["dev"][seq]


# ------------------------------------------------------------------ device-side helpers
def _poisoned(torch, payload):
    """`payload` (device uint8) with 64 bytes of 0xFF on both sides: (pointer, keep-alive)."""
    n = payload.numel()
    buf = torch.full((64 + n + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[64:64 + n] = payload
    return buf.data_ptr() + 64, buf


def _device_keys(torch, pool, sel, stride):
    """The keys pool[sel] built on the device by gathering: (key pointer, offsets pointer | None, stride, keep)."""
    if stride:
        rows = torch.from_numpy(np.frombuffer(b"".join(pool), np.uint8).reshape(len(pool), stride).copy()).cuda()
        payload = rows[sel].reshape(-1)
        ptr, buf = _poisoned(torch, payload)
        del payload
        return ptr, None, stride, (buf,)
    K = sel.numel()
    blob = torch.from_numpy(np.frombuffer(b"".join(pool) + b"\0", np.uint8).copy()).cuda()
    plen = torch.tensor([len(k) for k in pool], dtype=torch.int64).cuda()
    pstart = torch.cumsum(plen, 0) - plen
    lens = plen[sel]
    offs = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(lens, 0)
    total = int(offs[-1].item())
    owner = torch.repeat_interleave(torch.arange(K, device="cuda"), lens, output_size=total)
    src = pstart[sel][owner] + (torch.arange(total, device="cuda") - offs[owner])
    ptr, buf = _poisoned(torch, blob[src])
    return ptr, offs.data_ptr(), 0, (buf, offs)


def _i32(g):
    """A Guarded's payload as int32 (the library's u32: compared bit for bit, widened with & 0xFFFFFFFF)."""
    import torch

    return g.view.view(torch.int32)


class Run:
    """One adl_bloom_level_candidates_device call into four guarded buffers of exactly the promised sizes."""

    def __init__(self, torch, ab, lv, kp, op, K, stride, seq, cap, stream=None):
        wsb = ab.lib().adl_bloom_level_candidates_workspace_bytes(K)
        self.pb = gb.Guarded((K + 1) * 4, 4, name="pair_begin")
        self.pt = gb.Guarded(cap * 4, 4, name="pair_table")
        self.npairs = gb.Guarded(8, 8, name="num_pairs")
        self.ws = gb.Guarded(wsb, 256, name="workspace")
        self.args = (lv._h, kp, op, K, stride, seq, self.pb.ptr, self.pt.ptr, cap, self.npairs.ptr, self.ws.ptr, wsb)
        self.call = ab.lib().adl_bloom_level_candidates_device
        if stream is None:
            self.launch(None)
            torch.cuda.synchronize()
            self.check()

    def launch(self, sptr):
        rc = self.call(*self.args, sptr)
        assert rc == 0, rc

    def check(self):
        gb.check_all(self.pb, self.pt, self.npairs, self.ws)

    @property
    def num_pairs(self):
        return int(self.npairs.numpy().view(np.uint64)[0])


def _first(bad):
    """(count, index of the first) of a bool device tensor."""
    import torch

    n = int(bad.sum().item())
    return n, (int(bad.to(torch.uint8).argmax().item()) if n else -1)


def device_compare(torch, sel, len_of, lists, pb32=None, pt32=None, limit=None, chunk=1 << 18):
    """Where they live: pair_begin against cumsum(len_of[sel]) (64-bit, compared
    mod 2^32) and the first min(total, limit) entries of pair_table against a
    gather from `lists`, `chunk` keys at a time.  Only counts and first indices
    come back: {total, block_totals, begin_bad, begin_first, table_bad, table_first}."""
    K = sel.numel()
    lens = len_of[sel]
    begin = torch.zeros(K + 1, dtype=torch.int64, device=sel.device)
    begin[1:] = torch.cumsum(lens, 0)
    total = int(begin[-1].item())
    padded = torch.zeros(-(-K // KBLOCK) * KBLOCK, dtype=torch.int64, device=sel.device)
    padded[:K] = lens
    out = {"total": total, "block_totals": padded.view(-1, KBLOCK).sum(1), "begin_bad": 0, "begin_first": -1,
           "table_bad": 0, "table_first": -1}
    if pb32 is not None:
        assert pb32.numel() == K + 1
        out["begin_bad"], out["begin_first"] = _first((pb32.to(torch.int64) & 0xFFFFFFFF) != (begin & 0xFFFFFFFF))
    if pt32 is None:
        return out
    n_cmp = total if limit is None else min(total, int(limit))
    assert pt32.numel() >= n_cmp
    bounds = begin[torch.arange(0, K + chunk, chunk, device=sel.device).clamp(max=K)].cpu().tolist()
    for c, a in enumerate(range(0, K, chunk)):
        b = min(K, a + chunk)
        p0, p1 = bounds[c], bounds[c + 1]
        if p0 >= n_cmp:
            break
        if p1 == p0:
            continue
        owner = torch.repeat_interleave(torch.arange(a, b, device=sel.device), lens[a:b], output_size=p1 - p0)
        pos = torch.arange(p0, p1, device=sel.device) - begin[owner]
        want = lists[sel[owner], pos]
        m = min(p1, n_cmp) - p0
        nbad, first = _first(pt32[p0:p0 + m] != want[:m])
        if nbad and not out["table_bad"]:
            out["table_first"] = p0 + first
        out["table_bad"] += nbad
        del owner, pos, want
    return out


def _assert_equal(cmp, what):
    for name in ("begin", "table"):
        assert cmp[name + "_bad"] == 0, (f"{what}: {cmp[name + '_bad']} pair_{name} entries differ, "
                                         f"the first at {cmp[name + '_first']}")


def _reached(case, K, cmp, cap):
    nblk = -(-K // KBLOCK)
    w = min(cmp["total"], cap) - 1
    print(f"\nreached: {case}: K={K} nblk={nblk} per={-(-nblk // KBLOCK)} pairs={cmp['total']} "
          f"largest_w={w} largest_workgroup_total={int(cmp['block_totals'].max().item())}")


def _need(torch, nbytes, what):
    free, _ = torch.cuda.mem_get_info()
    assert free >= nbytes, f"{what} needs {nbytes / GIB:.1f} GiB of free device memory, {free / GIB:.1f} GiB are free"


# ------------------------------------------------------------------ 1. scan runs
@pytest.mark.parametrize("view", ("var", "stride16"))
@pytest.mark.parametrize("level", ("t16", "t300"))
@pytest.mark.parametrize("K", SCAN_KS)
def test_scan_runs(dev, ab, oracle, K, level, view):
    """level_scan_kernel with per = 1, 2, 2, 2, 3, 4 entries per thread and nblk
    = 256, 257, 257, 258, 513, 782: with 257 thread 128's run is clipped to one
    entry, with 782 thread 195's to two, and the threads behind them (129..,
    129.., 171.., 196..) own empty runs.  Full capacity, guard bands on all
    four buffers."""
    torch = dev
    stride = 16 if view == "stride16" else None
    case = _case(oracle, level, stride)
    lv = _index(ab, level)
    npool = len(case["pool"])
    sel = torch.from_numpy(_select(K, npool, SCAN_KS.index(K) * 7 + (level == "t300") * 3 + (stride or 0))).cuda()
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, stride)
    nblk = -(-K // KBLOCK)
    for seq in SEQS:
        len_of, lists = _expect(torch, case, seq)
        exp = device_compare(torch, sel, len_of, lists)
        bt = exp["block_totals"]
        assert bt.numel() == nblk and int(bt.min().item()) != int(bt.max().item()), "every workgroup total is the same"
        run = Run(torch, ab, lv, kp, op, K, st, seq, exp["total"])
        assert run.num_pairs == exp["total"]
        cmp = device_compare(torch, sel, len_of, lists, _i32(run.pb), _i32(run.pt))
        _assert_equal(cmp, f"K={K} {level} {view} seq={seq}")
        if seq == 25:
            _reached(f"scan runs {level} {view}", K, cmp, exp["total"])
    del keep


def test_scan_ks_reach_the_runs_named():
    """(K, nblk, per) of case 1, from the kernel's own arithmetic."""
    got = [(K, -(-K // KBLOCK), -(-(-(-K // KBLOCK)) // KBLOCK)) for K in SCAN_KS]
    assert got == [(65536, 256, 1), (65537, 257, 2), (65792, 257, 2), (65793, 258, 2), (131073, 513, 3),
                   (200001, 782, 4)]


def test_device_compare_sees_one_wrong_entry(dev, ab, oracle):
    """The comparer reports exactly the entry that was changed: one of
    pair_table (in the second chunk), one of pair_begin, and a list entry
    swapped with its neighbour."""
    torch = dev
    case = _case(oracle, "t300", None)
    lv = _index(ab, "t300")
    K = 65537
    sel = torch.from_numpy(_select(K, len(case["pool"]), 5)).cuda()
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, None)
    len_of, lists = _expect(torch, case, 25)
    total = device_compare(torch, sel, len_of, lists)["total"]
    run = Run(torch, ab, lv, kp, op, K, st, 25, total)
    pb, pt = _i32(run.pb).clone(), _i32(run.pt).clone()
    _assert_equal(device_compare(torch, sel, len_of, lists, pb, pt, chunk=20000), "untouched")
    at = total - 12345
    pt[at] += 1
    cmp = device_compare(torch, sel, len_of, lists, pb, pt, chunk=20000)
    assert (cmp["table_bad"], cmp["table_first"], cmp["begin_bad"]) == (1, at, 0)
    assert device_compare(torch, sel, len_of, lists, pb, pt, limit=at, chunk=20000)["table_bad"] == 0
    pt[at] -= 1
    pb[40001] += 1
    cmp = device_compare(torch, sel, len_of, lists, pb, pt)
    assert (cmp["begin_bad"], cmp["begin_first"], cmp["table_bad"]) == (1, 40001, 0)
    pb[40001] -= 1
    pt[7], pt[8] = pt[8].clone(), pt[7].clone()
    assert int(pt[7].item()) != int(pt[8].item())
    cmp = device_compare(torch, sel, len_of, lists, pb, pt)
    assert (cmp["table_bad"], cmp["table_first"]) == (2, 7)
    del keep


# ------------------------------------------------------------------ 2, 3. around 2^32 pairs
def _edge_pool():
    """One-byte keys for the all-overlap level t300: 0x65 (all 300 tables) first."""
    return [bytes([b]) for b in [0x65, 0x71, 0xff, 0x00, 0x70] + list(range(0x04, 0x60, 4))]


_edge = {}


def _edge_batches(torch, oracle):
    """sel_below: total in [2^32 - 300, 2^32); sel_above = sel_below and one more
    key of 300 candidates: total in [2^32, 2^32 + 300).  Made on the device:
    one key in 64 is drawn from the whole pool, the others are 0x65."""
    if not _edge:
        case = _case(oracle, "t300", 1, pool=_edge_pool(), check=False)
        len_of, _ = _expect(torch, case, 25)
        host_len = [len(x) for x in case["want"][25]]
        assert host_len[0] == 300 and 0 in host_len and any(0 < n < 300 for n in host_len)
        K0 = 14_200_000
        h = (torch.arange(K0, dtype=torch.int64, device="cuda") * 2654435761) & 0xFFFFFFFF
        sel = torch.where((h >> 26) == 0, (h >> 4) % len(case["pool"]), torch.zeros_like(h))
        t0 = int(len_of[sel].sum().item())
        tail = (2**32 - 1 - t0) // 300
        assert tail > 0
        below = torch.cat([sel, torch.zeros(tail, dtype=torch.int64, device="cuda")])
        _edge.update(case=case, below=below, above=torch.cat([below, torch.zeros(1, dtype=torch.int64, device="cuda")]))
    return _edge


@pytest.fixture(scope="module", autouse=True)
def _drop_edge():
    yield
    _edge.clear()


def test_just_below_2_32_pairs_capacity_4096(dev, ab, oracle):
    """*d_num_pairs and all of pair_begin exact (the last entries close to
    2^32), the first 4096 table entries exact, nothing written behind them."""
    torch = dev
    e = _edge_batches(torch, oracle)
    case, sel = e["case"], e["below"]
    K = sel.numel()
    len_of, lists = _expect(torch, case, 25)
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, 1)
    run = Run(torch, ab, _index(ab, "t300"), kp, op, K, st, 25, 4096)
    cmp = device_compare(torch, sel, len_of, lists, _i32(run.pb), _i32(run.pt), limit=4096)
    assert 2**32 - 300 <= cmp["total"] < 2**32
    assert run.num_pairs == cmp["total"]
    _assert_equal(cmp, "capacity 4096")
    bt = cmp["block_totals"]
    assert int(bt.min().item()) != int(bt.max().item())
    _reached("just below 2^32, capacity 4096", K, cmp, 4096)


def test_just_below_2_32_pairs_full_capacity(dev, ab, oracle):
    """The one case that writes pair_table at w close to 2^32: every entry
    compared, guard bands intact behind entry total - 1."""
    torch = dev
    e = _edge_batches(torch, oracle)
    case, sel = e["case"], e["below"]
    K = sel.numel()
    len_of, lists = _expect(torch, case, 25)
    total = device_compare(torch, sel, len_of, lists)["total"]
    assert 2**32 - 300 <= total < 2**32
    _need(torch, 4 * total + 6 * GIB, "a pair_table of 2^32 - x entries, and the comparison's chunks,")
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, 1)
    run = Run(torch, ab, _index(ab, "t300"), kp, op, K, st, 25, total)
    assert run.num_pairs == total
    cmp = device_compare(torch, sel, len_of, lists, _i32(run.pb), _i32(run.pt))
    _assert_equal(cmp, "full capacity")
    _reached("just below 2^32, full capacity", K, cmp, total)


def test_at_and_above_2_32_pairs(dev, ab, oracle):
    """*d_num_pairs exact as a u64; the first 4096 entries exact (pair_begin has
    not wrapped there); all guard bands intact.  Nothing is asserted about
    pair_begin: the header calls it meaningless from 2^32."""
    torch = dev
    e = _edge_batches(torch, oracle)
    case, sel = e["case"], e["above"]
    K = sel.numel()
    len_of, lists = _expect(torch, case, 25)
    kp, op, st, keep = _device_keys(torch, case["pool"], sel, 1)
    run = Run(torch, ab, _index(ab, "t300"), kp, op, K, st, 25, 4096)
    cmp = device_compare(torch, sel, len_of, lists, None, _i32(run.pt), limit=4096)
    assert 2**32 <= cmp["total"] < 2**32 + 300
    assert run.num_pairs == cmp["total"]
    _assert_equal(cmp, "capacity 4096")
    _reached("at and above 2^32, capacity 4096", K, cmp, 4096)


def test_multiget_status_on_both_sides_of_2_32_pairs(dev, ab, oracle):
    """adl_bloom_level_multiget on host copies of the two batches, capacity
    4096, no table cached: ADL_ERR_WORKSPACE just below 2^32 with *num_pairs
    exact and h_pair_begin complete and exact; ADL_ERR_TOO_LARGE from 2^32 with
    *num_pairs exact; h_pair_table and h_out untouched both times."""
    torch = dev
    e = _edge_batches(torch, oracle)
    case = e["case"]
    lv = _index(ab, "t300", oids=True)
    cache = ab.FilterCache(1 << 20, max_tables=16)
    try:
        assert cache.stats()[0] == 0
        host_len = np.array([len(x) for x in case["want"][25]], np.int64)
        pool_byte = np.frombuffer(b"".join(case["pool"]), np.uint8)
        for which, status in (("below", ab.ADL_ERR_WORKSPACE), ("above", ab.ADL_ERR_TOO_LARGE)):
            sel = e[which].cpu().numpy()
            K = len(sel)
            keys = pool_byte[sel]
            begin = np.zeros(K + 1, np.int64)
            np.cumsum(host_len[sel], out=begin[1:])
            total = int(begin[-1])
            assert (total < 2**32) == (which == "below") and abs(total - 2**32) <= 300
            pb = np.full(K + 1, 0xA5A5A5A5, np.uint32)
            pt = np.full(4096, 0xA5A5A5A5, np.uint32)
            out = np.full(4096, 0xA5, np.uint8)
            n, unc = ctypes.c_uint64(), ctypes.c_uint64()
            rc = ab.lib().adl_bloom_level_multiget(lv._h, cache._h, 0, keys.ctypes.data, None, K, 1, 25, pb.ctypes.data,
                                                   pt.ctypes.data, out.ctypes.data, 4096, ctypes.byref(n),
                                                   ctypes.byref(unc), None)
            assert rc == status, (which, rc)
            assert n.value == total, (which, n.value, total)
            if which == "below":
                b32 = begin.astype(np.uint32)
                assert np.array_equal(pb, b32), int(np.flatnonzero(pb != b32)[0])
            assert (pt == 0xA5A5A5A5).all() and (out == 0xA5).all(), which
    finally:
        cache.close()


# ------------------------------------------------------------------ 4. key bytes and offsets past 2^32
def test_key_bytes_past_2_32_at_stride_320(dev, ab, oracle):
    """KeySet::at's keys + i * stride beyond 4 GiB: the keys of the last 2^20
    bytes include keys that equal a (320-byte) boundary."""
    torch = dev
    stride = 320
    K = (2**32 + 2**20) // stride + 1
    assert K * stride > 2**32 + 2**20
    _need(torch, 2 * K * stride + 4 * GIB, "two copies of 4 GiB + 1 MiB of keys")
    case = _case(oracle, "t16+320", stride)
    pool, users = case["pool"], set(_boundaries(case["tables"]))
    lv = _index(ab, "t16+320")
    sel_h = _select(K, len(pool), 320)
    last = sel_h[K - 2**20 // stride:]  # the keys that lie wholly in the last 2^20 bytes
    assert (K - len(last)) * stride >= 2**32
    hits = [int(i) for i in set(last.tolist()) if pool[i] in users]
    assert hits and any(case["want"][24][i] != case["want"][26][i] for i in hits)
    sel = torch.from_numpy(sel_h).cuda()
    kp, op, st, keep = _device_keys(torch, pool, sel, stride)
    for seq in SEQS:
        len_of, lists = _expect(torch, case, seq)
        total = device_compare(torch, sel, len_of, lists)["total"]
        run = Run(torch, ab, lv, kp, op, K, st, seq, total)
        assert run.num_pairs == total
        cmp = device_compare(torch, sel, len_of, lists, _i32(run.pb), _i32(run.pt))
        _assert_equal(cmp, f"stride 320 seq={seq}")
        if seq == 25:
            _reached(f"stride 320, {K * stride} key bytes", K, cmp, total)
    del keep


def test_varlen_offsets_past_2_32(dev, ab, oracle):
    """Device u64 offsets beyond 2^32 and lengths just below 2^30: five filler
    keys of which only the first 17 bytes are written -- no boundary shares
    their first 16, so those alone place them -- and then the whole t16 pool."""
    torch = dev
    case = _case(oracle, "t16", None)
    tables, pool = case["tables"], case["pool"]
    lv = _index(ab, "t16")
    heads = [b"ab" + b"\x01" * 14 + b"\x07", P40[:15] + b"\x02\xee", b"\x7f\x11" + b"\x33" * 15,
             b"q" * 15 + b"\x91\x05", b"\xfe\x81" + b"\x44" * 15]
    users = _boundaries(tables)
    for h in heads:
        assert len(h) == 17 and 0 not in h[:16]  # (a shorter boundary's zero-padded prefix cannot equal it either)
        assert not any(u.startswith(h[:16]) for u in users)
    fill_len = [2**30 - 1 - j for j in range(len(heads))]
    lens = fill_len + [len(k) for k in pool]
    offs_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # the last filler straddles 2^32, every pool key lies beyond it
    assert offs_h[len(heads) - 1] < 2**32 < offs_h[len(heads)] and offs_h[len(heads)] > 5 * 2**30 - 64
    nbytes = int(offs_h[-1])
    _need(torch, nbytes + GIB, "an uninitialised key buffer of 5 GiB")
    buf = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
    for h, o in zip(heads, offs_h):
        buf[int(o):int(o) + 17] = torch.from_numpy(np.frombuffer(h, np.uint8).copy()).cuda()
    tail = np.frombuffer(b"".join(pool), np.uint8).copy()
    buf[int(offs_h[len(heads)]):nbytes] = torch.from_numpy(tail).cuda()
    offs = torch.from_numpy(offs_h).cuda()
    K = len(lens)
    some = 0
    for seq in SEQS:
        # (head + anything lies in head's region: no boundary begins with head)
        lists = [oracle.level_candidates(tables, h, seq) for h in heads] + case["want"][seq]
        begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
        flat = np.array([t for x in lists for t in x], np.uint32)
        run = Run(torch, ab, lv, buf.data_ptr(), offs.data_ptr(), K, 0, seq, len(flat))
        assert run.num_pairs == len(flat)
        got_b, got_t = run.pb.numpy().view(np.uint32), run.pt.numpy().view(np.uint32)
        assert np.array_equal(got_b, begin), (seq, int(np.flatnonzero(got_b != begin)[0]))
        assert np.array_equal(got_t, flat), (seq, int(np.flatnonzero(got_t != flat)[0]))
        some += sum(len(x) for x in lists[:len(heads)])
    assert some > 0  # the fillers do have candidates
    print(f"\nreached: var-len offsets: K={K} largest_offset={int(offs_h[-2])} largest_length={fill_len[0]}")


# ------------------------------------------------------------------ 5. long lists
def _nested_pool():
    wide = [b"p", b"q1", b"nz", b"n0999", b"n0999\0", b"w\xff"]  # at or after the last min, before the first max
    on_max = [b"x0000", b"x0001", b"x0500", b"x0999"]           # a table's max user key: a filtered list
    none = [b"a", b"m\xff", b"z", b"x1000"]
    return wide + on_max + none + [b"n0000", b"n0500", b"n0500\0", b"x0500\0", b"x0998\x80"]


@pytest.mark.parametrize("K", (257, 1000))
def test_lists_of_a_thousand(dev, ab, oracle, K):
    """1 000 nested tables: most keys have 1 000 candidates, so a workgroup's
    strided copy makes about 1 000 rounds; keys on a max user key are copied
    by their own lane, which drops entries by seq."""
    torch = dev
    pool = _nested_pool()
    case = _case(oracle, "nested", None, pool=pool, check=False)
    lv = _index(ab, "nested")
    assert lv.stats()[3] == 1000
    w24, w26 = case["want"][24], case["want"][26]
    assert all(len(w26[i]) == 1000 for i in range(6))
    assert any(w24[i] != w26[i] and len(w26[i]) > 500 for i in range(6, 10))
    assert all(not w26[i] for i in range(10, 14))
    rng = np.random.default_rng(K)
    sel_h = np.where(rng.random(K) < 0.88, rng.integers(0, 6, K), rng.integers(6, len(pool), K))
    sel_h[:len(pool)] = rng.permutation(len(pool))
    sel = torch.from_numpy(sel_h).cuda()
    kp, op, st, keep = _device_keys(torch, pool, sel, None)
    for seq in SEQS:
        len_of, lists = _expect(torch, case, seq)
        exp = device_compare(torch, sel, len_of, lists)
        assert int(exp["block_totals"].max().item()) > 200000
        run = Run(torch, ab, lv, kp, op, K, st, seq, exp["total"])
        assert run.num_pairs == exp["total"]
        cmp = device_compare(torch, sel, len_of, lists, _i32(run.pb), _i32(run.pt))
        _assert_equal(cmp, f"nested K={K} seq={seq}")
        if seq == 25:
            _reached("lists of 1 000", K, cmp, exp["total"])
    del keep


# ------------------------------------------------------------------ 6. empty shapes
@pytest.mark.parametrize("K", (1, 300))
@pytest.mark.parametrize("level", ("none", "inverted"))
def test_levels_without_candidates(dev, ab, oracle, level, K):
    """No table at all (NB = 0: rbeg has two entries), and eight tables with
    max < min (16 boundaries, every list empty)."""
    torch = dev
    tables = _tables(level)
    lv = _index(ab, level, oids=True)
    nb = len(_boundaries(tables))
    assert nb == 2 * len(tables)
    regions, entries, _, longest = lv.stats()
    assert (regions, entries, longest) == (2 * nb + 1, 0, 0)
    pool = sorted({b"", b"m", b"m00", b"m07", b"m07\0", b"m15", b"m16", b"\xff" * 20, P40})
    assert all(oracle.level_candidates(tables, k, 25) == [] for k in pool)
    keys = [pool[int(i)] for i in _select(K, len(pool), K)]
    sel = torch.from_numpy(np.array([pool.index(k) for k in keys])).cuda()
    kp, op, st, keep = _device_keys(torch, pool, sel, None)
    run = Run(torch, ab, lv, kp, op, K, st, 25, 1)
    assert run.num_pairs == 0
    assert not run.pb.numpy().any()
    assert (run.pt.numpy() == 0xA5).all()
    cache = ab.FilterCache(1 << 20, max_tables=16)
    try:
        data, offs = oracle.pack(keys)
        rc, pb, pt, out, n, unc = lv.multiget_status(cache, data, offs, seq=25)
        assert (rc, n, unc, len(pt), len(out)) == (0, 0, 0, 0, 0) and not pb.any() and len(pb) == K + 1
    finally:
        cache.close()
    del keep


# ------------------------------------------------------------------ 7. threads
def test_eight_threads_race_the_first_device_call(dev, ab, oracle):
    """One fresh level, no device call on it beforehand; a barrier releases
    four threads that select on streams of their own into guarded buffers and
    four that multi-get.  20 calls each, K alternating between 700 and 20 000,
    every result equal to what the oracle gave beforehand."""
    torch = dev
    universe, tabs = _multiget_level(oracle)
    tables = [t["range"] for t in tabs]
    oids = [t["oid"] for t in tabs]
    seq, calls, nthreads = 25, 20, 8
    cache = ab.FilterCache(16 << 20, max_tables=16)
    lv = ab.LevelIndex(tables, oids=oids)
    try:
        for t in tabs[:4]:
            cache.put(t["oid"], t["block"])
        cached = [True, True, True, True, False]
        rng = np.random.default_rng(7)
        pool = sorted({universe[int(i)] for i in rng.integers(0, len(universe), 1500)} |
                      {_user(r[1]) for r in tables} | {_user(r[0]) for r in tables} | {b"", b"\xff" * 41})
        per_pool = [oracle.level_candidates(tables, k, seq) for k in pool]
        batches = {}
        for K in (700, 20000):
            sel = _select(K, len(pool), K)
            keys = [pool[int(i)] for i in sel]
            lists = [per_pool[int(i)] for i in sel]
            begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
            flat = np.array([t for x in lists for t in x], np.uint32)
            data, offs = oracle.pack(keys)
            batches[K] = {"data": data, "offs": offs, "begin": begin, "flat": flat,
                          "answers": _expected_answers(oracle, tabs, keys, begin, flat, cached),
                          "uncached": int(sum(not cached[int(t)] for t in flat)),
                          "d_data": gb.Poisoned(data[:-1], 16),
                          "d_offs": torch.from_numpy(offs.astype(np.int64)).cuda()}
            assert batches[K]["uncached"] > 0 and 0 < int(batches[K]["answers"].sum()) < len(flat)
        before = (cache.stats(), [o in cache for o in oids])
        barrier = threading.Barrier(nthreads)
        errors = []

        class Selector:
            def __init__(self):
                self.stream = torch.cuda.Stream()
                self.runs = {K: Run(torch, ab, lv, b["d_data"].ptr, b["d_offs"].data_ptr(), K, 0, seq, len(b["flat"]),
                                    stream=self.stream) for K, b in batches.items()}

            def __call__(self, i):
                K = (700, 20000)[i & 1]
                run, b = self.runs[K], batches[K]
                with torch.cuda.stream(self.stream):
                    run.pb.view.zero_(), run.pt.view.zero_(), run.npairs.view.zero_()
                    run.launch(ctypes.c_void_p(self.stream.cuda_stream))
                    got = (run.pb.numpy().view(np.uint32), run.pt.numpy().view(np.uint32), run.num_pairs)
                assert got[2] == len(b["flat"]), (K, got[2])
                assert np.array_equal(got[0], b["begin"]) and np.array_equal(got[1], b["flat"]), K

        def multiget(i):
            K = (700, 20000)[i & 1]
            b = batches[K]
            rc, pb, pt, out, n, unc = lv.multiget_status(cache, b["data"], b["offs"], seq=seq)
            assert (rc, n, unc) == (0, len(b["flat"]), b["uncached"]), (K, rc, n, unc)
            assert np.array_equal(pb, b["begin"]) and np.array_equal(pt, b["flat"]), K
            assert np.array_equal(out, b["answers"]), K

        selectors = [Selector() for _ in range(4)]
        torch.cuda.synchronize()

        def worker(t, call):
            try:
                barrier.wait(timeout=60)
                for i in range(calls):
                    call(i + t)
            except BaseException as e:  # noqa: BLE001 (reported by the main thread)
                errors.append((t, repr(e)))

        threads = [threading.Thread(target=worker, args=(t, selectors[t] if t < 4 else multiget), daemon=True)
                   for t in range(nthreads)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
        if any(th.is_alive() for th in threads):
            pytest.exit("a thread of the level-index race did not finish: nothing more is started on the GPU", 1)
        assert not errors, errors
        torch.cuda.synchronize()
        for s in selectors:
            for run in s.runs.values():
                run.check()
        assert (cache.stats(), [o in cache for o in oids]) == before
    finally:
        lv.close()
        cache.close()


# ------------------------------------------------------------------ 8. the same race through the C++ class
def test_level_index_binary_race(dev):
    """bin/level_index_test --race: eight threads whose first call on one
    shared LevelIndex is the 3 000-key device path (handle()'s call_once and
    the upload race); every MultiGetFilterResult equals
    LevelMultiGetFilter(cache, tables, ...)."""
    exe = os.path.join(ROOT, "adlsm-tree_amd", "bin", "level_index_test")
    assert os.path.exists(exe), f"{exe} is missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if k != "ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS"}
    r = subprocess.run([exe, "--race"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
