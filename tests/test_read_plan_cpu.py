"""CPU: the read plan (adlsm-tree_amd/csrc/read_plan.hip,
adl_bloom_revision_read_plan) as far as it needs no GPU, and the host grouping
of the C++ mirror.

* the symbols exist in the library and in EXPORTS, ADL_BLOOM_ABI_VERSION is
  unchanged, HITS_TILE is exported;
* adl_bloom_hits_by_table_workspace_bytes is monotone in each argument, grows
  by a tile's histogram at every multiple of HITS_TILE, and is 0 for an
  entry_capacity of 2^32 or more;
* the device entry points check their arguments before they touch a device;
* GroupHitsByTable (adl_revision_group_hits) against numpy (a stable argsort of
  the table ids, np.unique for the groups) on the candidate lists of
  revisionkeys.REVISIONS["five"] under random keep masks, on no hits, on every
  hit in one table, and with keys without hits at the front, in the middle and
  at the end.
The expectation never comes from the code under test."""
import ctypes
import os

import numpy as np
import pytest

import revisionkeys as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIRROR = os.path.join(ROOT, "adlsm-tree_amd", "lib", "libadlfilterblock.so")
NEW = ("adl_bloom_hits_by_table_workspace_bytes", "adl_bloom_hits_by_table_device", "adl_bloom_revision_read_plan")
INVALID_ARG, TOO_LARGE, WORKSPACE = -1, -2, -5


def expected_plan(hit_begin, hit_table):
    """numpy's grouping of a key-major hit list: (group_table, group_begin, entry_key)."""
    hit_begin = np.asarray(hit_begin, np.int64)
    hit_table = np.asarray(hit_table, np.uint32)
    owner = np.repeat(np.arange(len(hit_begin) - 1), np.diff(hit_begin)).astype(np.uint32)
    order = np.argsort(hit_table, kind="stable")
    tabs, counts = np.unique(hit_table, return_counts=True)
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return tabs.astype(np.uint32), begin, owner[order]


@pytest.fixture(scope="module")
def ab():
    import adlbloom

    adlbloom.lib()
    return adlbloom


def test_symbols_and_abi_version(ab):
    L = ab.lib()
    for name in NEW:
        assert hasattr(L, name) and name in ab.EXPORTS, name
    assert L.adl_bloom_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "adl_bloom.h")).read()
    assert "#define ADL_BLOOM_ABI_VERSION 1\n" in header
    assert ab.HITS_TILE == 2048
    for name in ("hits_by_table",):
        assert callable(getattr(ab, name))
    assert callable(ab.Revision.read_plan) and callable(ab.Revision.read_plan_status)


def test_workspace_bytes(ab):
    f = ab.lib().adl_bloom_hits_by_table_workspace_bytes
    E = ab.HITS_TILE
    caps = (0, 1, E - 1, E, E + 1, 3 * E + 17, 300 * E + 5, 2**32 - 1)
    tables = (0, 1, 2, 256, 257, 65536, 65537, 2**24 + 1, 2**32 - 1)
    keys = (0, 1, 1000, 2**32 - 2)
    for k in keys:
        for t in tables:
            w = [f(k, c, t) for c in caps]
            assert w[0] > 0 and all(a <= b for a, b in zip(w, w[1:])), (k, t, w)
            assert all(x % 256 == 0 for x in w)
    for k in keys:
        for c in caps:
            w = [f(k, c, t) for t in tables]
            assert all(a <= b for a, b in zip(w, w[1:])), (k, c, w)
    for c in caps:
        for t in tables:
            w = [f(k, c, t) for k in keys]
            assert all(a <= b for a, b in zip(w, w[1:])), (c, t, w)
    # the sorted ids and keys of every entry, and a 256-counter histogram per tile: one more tile, 1 KiB more
    assert f(1000, 10 * E, 256) >= 2 * 4 * 10 * E + 10 * 1024
    assert f(1000, 10 * E + 1, 256) >= f(1000, 10 * E, 256) + 1024
    # a second pass needs the second pair of buffers
    assert f(1000, 10 * E, 257) >= f(1000, 10 * E, 256) + 2 * 4 * 10 * E
    assert f(1000, 2**32, 256) == 0 and f(1000, 2**40, 1) == 0


def test_argument_checks(ab):
    """Refusals that are decided before any device is touched."""
    L = ab.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    wsb = L.adl_bloom_hits_by_table_workspace_bytes(4, 8, 16)
    assert wsb <= (1 << 16) - 512

    def call(hb=p, ht=p, K=4, T=16, gt=p, gb=p, gcap=8, ek=p, ecap=8, counts=p, ws=p, wbytes=wsb):
        return L.adl_bloom_hits_by_table_device(hb, ht, K, T, gt, gb, gcap, ek, ecap, counts, ws, wbytes, None)

    assert call(K=2**32 - 1) == TOO_LARGE
    assert call(K=2**40) == TOO_LARGE
    assert call(ecap=2**32) == TOO_LARGE
    assert call(wbytes=wsb - 1) == WORKSPACE
    assert call(ws=p + 64) == INVALID_ARG
    assert call(ws=None) == INVALID_ARG
    assert call(hb=None) == INVALID_ARG
    assert call(gb=None) == INVALID_ARG
    assert call(counts=None) == INVALID_ARG
    assert call(ht=None) == INVALID_ARG and call(ek=None) == INVALID_ARG and call(gt=None) == INVALID_ARG
    n = [ctypes.c_uint64() for _ in range(4)]
    assert L.adl_bloom_revision_read_plan(None, None, 0, p, None, 1, 16, 0, p, p, 1, ctypes.byref(n[0]), p, 1,
                                          ctypes.byref(n[1]), 0, ctypes.byref(n[2]), ctypes.byref(n[3]),
                                          None) == INVALID_ARG


@pytest.fixture(scope="module")
def group_hits():
    if not os.path.exists(MIRROR):
        pytest.fail(f"{MIRROR} is missing: run __graft_entry__.build()")
    f = ctypes.CDLL(MIRROR).adl_revision_group_hits
    f.restype = ctypes.c_int64
    vp = ctypes.c_void_p
    f.argtypes = [vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp]

    def run(hit_begin, hit_table, table_base, group_cap=None):
        hb = np.ascontiguousarray(hit_begin, np.uint32)
        ht = np.ascontiguousarray(np.concatenate([hit_table, [0]]), np.uint32)
        base = np.ascontiguousarray(table_base, np.uint32)
        K, L, H = len(hb) - 1, len(base) - 1, int(hb[-1])
        cap = int(base[-1]) if group_cap is None else group_cap
        gt = np.full(cap + 1, 0xA5A5A5A5, np.uint32)
        gl = np.full(cap + 1, 0xA5, np.uint8)
        gb = np.full(cap + 2, 0xA5A5A5A5, np.uint32)
        key = np.full(H + 1, 0xA5A5A5A5, np.uint32)
        lb = np.full(L + 2, 0xA5A5A5A5, np.uint32)
        G = f(hb.ctypes.data, ht.ctypes.data, K, base.ctypes.data, L, gt.ctypes.data, gl.ctypes.data, gb.ctypes.data, cap,
              key.ctypes.data, lb.ctypes.data)
        if G < 0:
            return G, None
        # nothing past what the plan holds
        assert gt[G:].tolist() == [0xA5A5A5A5] * (cap + 1 - G) and key[H] == 0xA5A5A5A5 and lb[L + 1] == 0xA5A5A5A5
        assert gb[G + 1] == 0xA5A5A5A5 and gl[G:].tolist() == [0xA5] * (cap + 1 - G)
        return G, (gt[:G], gl[:G], gb[:G + 1], key[:H], lb[:L + 1])

    return run


def _check_grouping(run, hit_begin, hit_table, base):
    G, (gt, gl, gb, key, lb) = run(hit_begin, hit_table, base)
    want_t, want_b, want_k = expected_plan(hit_begin, hit_table)
    assert G == len(want_t)
    assert np.array_equal(gt, want_t) and np.array_equal(gb, want_b) and np.array_equal(key, want_k)
    base = np.asarray(base, np.int64)
    want_l = np.searchsorted(base, want_t.astype(np.int64), side="right") - 1
    assert np.array_equal(gl, want_l.astype(np.uint8))
    assert np.array_equal(lb, np.searchsorted(want_l, np.arange(len(base))).astype(np.uint32))
    return G


def test_group_hits_on_revision_lists(group_hits, oracle):
    names = rk.REVISIONS["five"]
    base = rk.table_base(names)
    keys = rk.pool(names)
    rng = np.random.default_rng(11)
    for seq, keep_p in ((25, 1.0), (26, 0.5), (24, 0.1), (2**63 - 1, 0.9)):
        begin, flat = rk.csr(rk.revision_lists(oracle, names, keys, seq))
        keep = rng.random(len(flat)) < keep_p
        owner = np.repeat(np.arange(len(keys)), np.diff(begin.astype(np.int64)))
        hb = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=len(keys)))]).astype(np.uint32)
        G = _check_grouping(group_hits, hb, flat[keep], base)
        assert G > 3 and len(set(np.searchsorted(base, np.unique(flat[keep]), side="right"))) > 1  # several levels


def test_group_hits_edges(group_hits):
    base = [0, 3, 3, 3, 19, 319]
    # no hits; no keys
    assert _check_grouping(group_hits, np.zeros(8, np.uint32), np.zeros(0, np.uint32), base) == 0
    assert _check_grouping(group_hits, np.zeros(1, np.uint32), np.zeros(0, np.uint32), base) == 0
    # every hit in one table (the last one)
    assert _check_grouping(group_hits, np.arange(501, dtype=np.uint32), np.full(500, 318, np.uint32), base) == 1
    # keys without hits at the front, in the middle and at the end
    rng = np.random.default_rng(12)
    cnt = np.zeros(1000, np.int64)
    cnt[300:450] = rng.integers(1, 6, 150)
    cnt[600:700] = rng.integers(0, 3, 100)
    hb = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    lists = [rng.choice(319, int(c), replace=False) for c in cnt]  # (no table twice in a key's list)
    ht = np.concatenate(lists).astype(np.uint32)
    G = _check_grouping(group_hits, hb, ht, base)
    assert G > 100
    # a group capacity that is too small is refused
    assert group_hits(hb, ht, base, group_cap=G - 1)[0] == -1
