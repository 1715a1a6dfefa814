"""GPU: the fan-out probe -- each key once against a list of filters
(Level::Get's shape, src/revision.cpp:265-310) -- through the device API, the
filter cache and LevelMultiGetFilter.

Every expected answer comes from the oracle on the EXPANDED pairs
(oracle.probe_multi / oracle.probe: one independent query per (key, filter)
pair), so the fan-out path must equal the pair path bit for bit: a filter id
>= num_filters and an empty filter answer 0.

* Device API: 1 / 255 / 256 / 257 / 1000 keys (one key block, its edges, four
  blocks), five fan-out patterns (none, random 0..8, one key with 700
  candidates at index 255 or 256 among keys with none, everything on the last
  key), five key views, four filter layouts (1, 3, 3 + an empty one, 4097: past
  the divisor table in LDS) and bits_per_key 0 / 3 / 10 / 44.
* Cache API: blocks of bits_per_key 3, 10 and 16 in one cache, an uncached
  table, a filter index the blocks lack, batches of <= 8 pairs (delegated to
  adl_bloom_filter_cache_probe: the resident server, or a launch), the mapped
  and the staged batch sizes, and the host-side validation.
* C++: bin/level_fanout_test with the fan-out path (ADL_BLOOM_LEVEL_FANOUT=1,
  the default, and 2, forced) and with the pair path (0) writes the same
  multi-get, which equals the oracle's candidates and answers."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL = 1000      # keys per view; the first MEMBERS of them are inserted into filters
MEMBERS = 600
KS = (1, 255, 256, 257, 1000)
PATTERNS = ("none", "random", "hot255", "hot256", "last")
BPKS = (0, 3, 10, 44)
VIEWS = ("k16", "k16_off1", "stride8", "stride24", "var")
LAYOUTS = ("f1", "f3", "f3_empty", "f4097")


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


def _pool(view):
    """POOL distinct keys of the view, as a list of bytes."""
    rng = np.random.default_rng(VIEWS.index(view) + 17)
    if view == "var":
        # every len % 4, a zero-length key, bytes >= 0x80
        keys = {b""}
        while len(keys) < POOL:
            n = int(rng.integers(1, 41))
            keys.add((rng.integers(0, 256, n, dtype=np.uint8) | (0x80 if len(keys) % 2 else 0)).astype(np.uint8).tobytes())
        keys = sorted(keys)
        rng.shuffle(keys)
        assert {len(k) % 4 for k in keys} == {0, 1, 2, 3} and b"" in keys
        return [bytes(k) for k in keys]
    stride = {"k16": 16, "k16_off1": 16, "stride8": 8, "stride24": 24}[view]
    a = rng.integers(0, 256, (POOL, stride), dtype=np.uint8)
    a[:, 0] = np.arange(POOL) & 0xFF  # distinct
    a[:, 1] = np.arange(POOL) >> 8
    return [r.tobytes() for r in a]


def _filters(oracle, pool, layout, bpk):
    """(bitmaps u8, off u64[F+1], ids drawn from [0, idmax)): members pool[:MEMBERS] spread over the filters."""
    if layout == "f4097":
        sets = [[pool[(8 * f + j) % MEMBERS] for j in range(8)] for f in range(4097)]
    else:
        F = 1 if layout == "f1" else 3
        sets = [pool[f:MEMBERS:F] for f in range(F)]
    bms = [oracle.keys2block(s, bits_per_key=bpk).tobytes() for s in sets]
    idmax = len(bms)
    if layout == "f3_empty":
        bms.insert(2, b"")     # a 0-byte filter: answers 0
        idmax = len(bms) + 2   # and ids >= num_filters: answer 0
    elif layout == "f4097":
        idmax = len(bms) + 1
    off = np.concatenate([[0], np.cumsum([len(b) for b in bms])]).astype(np.uint64)
    return np.frombuffer(b"".join(bms) + bytes(16), np.uint8), off, idmax


def _fanout(rng, K, pattern):
    cnt = np.zeros(K, np.int64)
    if pattern == "random":
        cnt = rng.integers(0, 9, K)
    elif pattern in ("hot255", "hot256"):
        cnt[min(int(pattern[3:]), K - 1)] = 700  # > 2 rounds of 256 lanes; 255 | 256 is a key-block edge
    elif pattern == "last":
        cnt[K - 1] = 300
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)


def _device_keys(torch, view, keys):
    """list[bytes] of the view -> (keys tensor, offsets tensor | None)."""
    if view == "var":
        offs = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
        data = np.frombuffer(b"".join(keys) + bytes(16), np.uint8).copy()
        return torch.from_numpy(data).cuda(), torch.from_numpy(offs).cuda()
    stride = len(keys[0])
    flat = np.frombuffer(b"".join(keys), np.uint8).copy()
    lead = 1 if view == "k16_off1" else 0
    buf = torch.empty(lead + flat.size + 16, dtype=torch.uint8, device="cuda")
    buf[lead:lead + flat.size] = torch.from_numpy(flat).cuda()
    t = buf[lead:lead + flat.size].view(len(keys), stride)
    assert t.data_ptr() % 16 == lead  # k16: the aligned 16-byte view; k16_off1: the byte-wise one
    return t, None


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("view", VIEWS)
def test_probe_fanout_device_vs_oracle(dev, ab, oracle, view, layout):
    torch = dev
    pool = _pool(view)
    rng = np.random.default_rng(VIEWS.index(view) * 10 + LAYOUTS.index(layout))
    checked = hits = zero_by_rule = 0
    for bpk in BPKS:
        bm, off, idmax = _filters(oracle, pool, layout, bpk)
        d_bm = torch.from_numpy(bm.copy()).cuda()
        d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
        F = len(off) - 1
        for K in KS:
            for pattern in PATTERNS:
                sel = rng.integers(0, POOL, K)
                keys = [pool[i] for i in sel]
                pb = _fanout(rng, K, pattern)
                P = int(pb[-1])
                pf = rng.integers(0, idmax, P).astype(np.uint32)
                owner = np.repeat(np.arange(K), np.diff(pb.astype(np.int64)))
                want = oracle.probe_multi([keys[i] for i in owner], pf, bm, off, bits_per_key=bpk) if P else \
                    np.empty(0, np.uint8)
                dk, do = _device_keys(torch, view, keys)
                got = ab.probe_fanout(dk, torch.from_numpy(pb.view(np.int32).copy()).cuda(),
                                      torch.from_numpy(pf.view(np.int32).copy()).cuda(), d_bm, d_off, offsets=do,
                                      bits_per_key=bpk)
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                assert got.shape == (P,), (bpk, K, pattern)
                assert np.array_equal(got, want), (bpk, K, pattern, int((got != want).sum()))
                checked += P
                hits += int(want.sum())
                if P:
                    empty = (pf >= F) | (np.diff(off)[np.minimum(pf, F - 1)] == 0)
                    assert not want[empty].any()
                    zero_by_rule += int(empty.sum())
    assert checked > 20000 and 0 < hits < checked
    if layout == "f3_empty":
        assert zero_by_rule > 1000


def _varlen_block(oracle, seed, n, bpk):
    rng = np.random.default_rng(seed)
    keys = [rng.integers(0, 256, int(rng.integers(0, 65)), dtype=np.uint8).tobytes() for _ in range(n)]
    bm = oracle.keys2block(keys, bits_per_key=bpk)
    return keys, oracle.filter_block_final([bm.tobytes()], bpk), bm


@pytest.fixture(scope="module")
def level(ab, oracle, dev):
    """Five cached tables (bits_per_key 3, 10, 16, 10, 3) and one oid that is not cached."""
    bpks = [3, 10, 16, 10, 3]
    tabs = [_varlen_block(oracle, 900 + t, 2000, b) for t, b in enumerate(bpks)]
    cache = ab.FilterCache(16 << 20, max_tables=16)
    oids = [b"fan-%d" % t for t in range(len(bpks))] + [b"fan-not-cached"]
    for o, (_, blk, _) in zip(oids, tabs):
        cache.put(o, blk)
    yield cache, oids, tabs, bpks
    cache.close()


def _level_batch(oracle, level, rng, K, cnt=None):
    """K var-len keys with candidate lists (cnt[i] distinct tables for key i,
    default random 0..5) over the six oids; the oracle's answer per expanded
    pair (1 for the uncached table)."""
    cache, oids, tabs, bpks = level
    T = len(tabs)
    keys = []
    for i in range(K):
        t = int(rng.integers(0, T))
        keys.append(tabs[t][0][int(rng.integers(0, 2000))] if i % 2 else
                    rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8).tobytes())
    cnt = rng.integers(0, 6, K) if cnt is None else np.asarray(cnt, np.int64)
    pb = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    pt = np.concatenate([rng.permutation(T + 1)[:c] for c in cnt] + [np.empty(0, np.int64)]).astype(np.uint32)
    owner = np.repeat(np.arange(K), cnt)
    ekeys = [keys[i] for i in owner]
    want = np.ones(len(pt), np.uint8)
    for t in range(T):
        s = np.flatnonzero(pt == t)
        if len(s):
            want[s] = oracle.probe([ekeys[i] for i in s], tabs[t][2], bits_per_key=bpks[t])
    return keys, ekeys, pb, pt, want


@pytest.mark.parametrize("K", [300, 6000], ids=["mapped", "staged"])
def test_cache_probe_fanout_vs_oracle_and_pair_path(ab, oracle, level, K):
    """K = 300: the batch fits the mapped buffer (answers watched); 6000: staged copies."""
    cache, oids, tabs, bpks = level
    rng = np.random.default_rng(K)
    keys, ekeys, pb, pt, want = _level_batch(oracle, level, rng, K)
    data, offs = oracle.pack(keys)
    got, unc = cache.probe_fanout(oids, pb, pt, data, offs)
    assert np.array_equal(got, want), int((got != want).sum())
    assert unc == int((pt == len(tabs)).sum()) and unc > 0
    assert 0 < int(want[pt < len(tabs)].sum()) < int((pt < len(tabs)).sum())
    edata, eoffs = oracle.pack(ekeys)
    pair, unc2 = cache.probe(oids, pt, edata, eoffs)
    assert got.tobytes() == pair.tobytes() and unc2 == unc
    # filter 1: these one-filter blocks do not have it (0); the uncached table still answers 1
    got1, unc1 = cache.probe_fanout(oids, pb, pt, data, offs, filter=1)
    assert np.array_equal(got1, (pt == len(tabs)).astype(np.uint8)) and unc1 == unc


def test_cache_probe_fanout_fixed_stride_keys(ab, oracle, dev):
    """16-byte keys handed over with a stride (no offsets), blocks of two bits_per_key."""
    tabs = []
    for t, bpk in enumerate((10, 16, 3)):
        k = oracle.splitmix_keys16(700 + t, 3000)
        bm = oracle.keys2block(k, bits_per_key=bpk)
        tabs.append((k, oracle.filter_block_final([bm.tobytes()], bpk), bm, bpk))
    cache = ab.FilterCache(8 << 20, max_tables=8)
    oids = [b"s-%d" % t for t in range(3)]
    for o, tb in zip(oids, tabs):
        cache.put(o, tb[1])
    rng = np.random.default_rng(3)
    K = 2500
    q = np.where((rng.integers(0, 2, K) == 1)[:, None], tabs[1][0][:K], oracle.splitmix_keys16(0xFA9, K))
    cnt = rng.integers(0, 4, K)
    pb = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    pt = np.concatenate([rng.permutation(3)[:c] for c in cnt]).astype(np.uint32)
    owner = np.repeat(np.arange(K), cnt)
    want = np.empty(len(pt), np.uint8)
    for t in range(3):
        s = pt == t
        want[s] = oracle.probe(q[owner[s]], tabs[t][2], bits_per_key=tabs[t][3])
    got, unc = cache.probe_fanout(oids, pb, pt, q)
    cache.close()
    assert unc == 0 and np.array_equal(got, want)
    assert 0 < int(want.sum()) < len(want)


@pytest.mark.parametrize("server", ["1", "0"])
def test_cache_probe_fanout_small_batches_delegate(ab, oracle, level, knobs, server):
    """Up to 8 pairs: expanded and answered by adl_bloom_filter_cache_probe (the
    resident server, or with ADL_BLOOM_PROBE_SERVER=0 a launched probe)."""
    cache, oids, tabs, bpks = level
    knobs.set("ADL_BLOOM_PROBE_SERVER", server)
    rng = np.random.default_rng(int(server) + 40)
    seen = set()
    fixed = [[0], [1], [6], [0, 0, 1], [2, 2, 2, 2], [5, 3], [0, 4, 0, 4, 0]]
    for it in range(120):
        cnt = fixed[it] if it < len(fixed) else rng.integers(0, 3, 1 + it % 4)
        keys, ekeys, pb, pt, want = _level_batch(oracle, level, rng, len(cnt), cnt)
        assert len(pt) <= 8
        data, offs = oracle.pack(keys)
        got, unc = cache.probe_fanout(oids, pb, pt, data, offs)
        assert np.array_equal(got, want), (it, got, want)
        assert unc == int((pt == len(tabs)).sum())
        seen.add(len(pt))
    assert {0, 1, 8} <= seen


def test_cache_probe_fanout_rejects_bad_lists(ab, oracle, level):
    cache, oids, tabs, bpks = level
    keys = [b"a", b"bb", b"ccc"] * 5
    data, offs = oracle.pack(keys)
    pb = np.arange(16, dtype=np.uint32)            # one candidate per key
    pt = np.zeros(15, np.uint32)
    got, _ = cache.probe_fanout(oids, pb, pt, data, offs)
    assert got.shape == (15,)
    bad = pb.copy()
    bad[7], bad[8] = 9, 8                          # decreasing inside, the end still 15
    with pytest.raises(ab.AdlBloomError) as e:
        cache.probe_fanout(oids, bad, pt, data, offs)
    assert e.value.status == -1
    bad = pb.copy()
    bad[0] = 1                                     # does not start at 0
    with pytest.raises(ab.AdlBloomError) as e:
        cache.probe_fanout(oids, bad, pt, data, offs)
    assert e.value.status == -1
    bad_t = pt.copy()
    bad_t[14] = len(oids)                          # a table index past the oid list
    with pytest.raises(ab.AdlBloomError) as e:
        cache.probe_fanout(oids, pb, bad_t, data, offs)
    assert e.value.status == -1
    got2, _ = cache.probe_fanout(oids, pb, pt, data, offs)  # and the cache still answers
    assert np.array_equal(got, got2)


def _run_level_fanout(out_dir, fanout):
    exe = os.path.join(ROOT, "adlsm-tree_amd", "bin", "level_fanout_test")
    os.makedirs(out_dir)
    r = subprocess.run([exe, str(out_dir)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ADL_BLOOM_LEVEL_FANOUT=fanout))
    assert r.returncode == 0, r.stdout + r.stderr
    return out_dir


def test_level_multiget_fanout_equals_pair_path_and_oracle(dev, oracle, tmp_path):
    """Switch 1 (the default: fan-out where it saves upload, as it does for this
    level), 2 (fan-out always) and 0 (the pair path)."""
    on = _run_level_fanout(tmp_path / "fanout", "1")
    forced = _run_level_fanout(tmp_path / "forced", "2")
    off = _run_level_fanout(tmp_path / "pairs", "0")
    assert (on / "multiget.txt").read_bytes() == (off / "multiget.txt").read_bytes()
    assert (forced / "multiget.txt").read_bytes() == (off / "multiget.txt").read_bytes()

    tables = []
    for line in (on / "tables.txt").read_text().split("\n"):
        if line:
            oid, mn, mx = line.split()
            tables.append((bytes.fromhex(mn), bytes.fromhex(mx)))
    assert len(tables) == 12
    readers = []
    for t in range(len(tables)):
        rd = oracle.FilterBlockReaderOracle()
        assert rd.init((on / f"table_{t}.blk").read_bytes()) == 0
        readers.append(rd)
    assert sorted({rd.bits_per_key for rd in readers}) == [3, 10, 16]
    queries = [bytes.fromhex(x) for x in (on / "queries.txt").read_text().split("\n") if x]
    assert len(queries) == 3000 and {len(q) for q in queries} == {16}
    got = {}
    for line in (on / "multiget.txt").read_text().split("\n"):
        if line:
            f = line.split()
            got[int(f[0])] = [(int(p.split(":")[0]), int(p.split(":")[1])) for p in f[1:]]
    assert len(got) == len(queries)
    want_bits = []
    for rd in readers:
        o1, o2 = rd.filter_range(0)
        want_bits.append(oracle.probe(queries, np.frombuffer(rd.block[o1:o2], dtype=np.uint8),
                                      bits_per_key=rd.bits_per_key))
    pairs = hits = 0
    for i, q in enumerate(queries):
        assert [t for t, _ in got[i]] == oracle.level_candidates(tables, q, 2**63 - 1), i
        for t, m in got[i]:
            assert m == want_bits[t][i], (i, t)
            pairs += 1
            hits += m
    assert pairs > len(queries)
    assert 0 < hits < pairs
