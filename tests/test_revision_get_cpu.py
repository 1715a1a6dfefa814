"""CPU: the single-key revision Get's GPU-free parts.

* adl_bloom_filter_cache_probe_key, adl_bloom_revision_candidates_host,
  adl_bloom_revision_get and the server-side limits exist; the ABI version is
  unchanged;
* the argument refusals of adl_bloom_revision_get, adl_bloom_filter_cache_probe_key
  and adl_bloom_revision_candidates_host that need no GPU;
* adl_bloom_revision_candidates_host equals oracle.level_candidates
  concatenated over the levels as global ids, on the five-level revision of
  tests/revisionkeys.py (an empty and a missing level) at seq 0, 24, 25, 26 and
  2^63-1, for the pool's keys (every boundary user key among them) and keys of
  every length 0-17, with `capacity` exact, one short and 0;
* the case table of tests/getkeys.py holds what it claims: every expectation
  is the oracle's, "exactly table j" is one-hot, every length and count the
  GPU test must send is there, and which calls fit one server request.
No call here reaches the GPU: the device copies are made by the first device call."""
import ctypes
import os

import numpy as np
import pytest

import getkeys as GK
import revisionkeys as rk
import serverkeys as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adl_bloom_filter_cache_probe_key", "adl_bloom_revision_candidates_host", "adl_bloom_revision_get")
INVALID_ARG = -1
SEQS = (0, 24, 25, 26, 2**63 - 1)


@pytest.fixture(scope="module")
def ab():
    import adlbloom

    adlbloom.lib()
    return adlbloom


@pytest.fixture(scope="module")
def five(ab):
    names = rk.REVISIONS["five"]
    levels = [None if n is None else ab.LevelIndex(rk.tables(n), oids=[b"five-%s-%d" % (n.encode(), t)
                                                                        for t in range(len(rk.tables(n)))])
              for n in names]
    rev = ab.Revision(levels)
    yield names, rev
    rev.close()
    for lv in levels:
        if lv is not None:
            lv.close()


def test_symbols_constants_and_abi_version(ab):
    L = ab.lib()
    for name in NEW:
        assert hasattr(L, name) and name in ab.EXPORTS, name
    assert L.adl_bloom_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "adl_bloom.h")).read()
    assert "#define ADL_BLOOM_GET_MAX_TABLES 24\n" in header and "#define ADL_BLOOM_GET_MAX_KEY_BYTES 96\n" in header
    assert (ab.GET_MAX_TABLES, ab.GET_MAX_KEY_BYTES) == (24, 96) == (GK.MAX_TABLES, GK.MAX_KEY_BYTES)
    for name in ("probe_key",):
        assert callable(getattr(ab.FilterCache, name))
    for name in ("candidates_host", "get", "get_status"):
        assert callable(getattr(ab.Revision, name))


def test_argument_refusals(ab, five):
    L = ab.lib()
    _, rev = five
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    n32, c32, u32 = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    # adl_bloom_revision_candidates_host
    assert L.adl_bloom_revision_candidates_host(None, p, 2, 0, p, 4, ctypes.byref(n32)) == INVALID_ARG
    assert L.adl_bloom_revision_candidates_host(rev._h, p, 2, 0, p, 4, None) == INVALID_ARG
    assert L.adl_bloom_revision_candidates_host(rev._h, None, 2, 0, p, 4, ctypes.byref(n32)) == INVALID_ARG
    assert L.adl_bloom_revision_candidates_host(rev._h, p, 2, 0, None, 4, ctypes.byref(n32)) == INVALID_ARG
    assert L.adl_bloom_revision_candidates_host(rev._h, None, 0, 0, None, 0, ctypes.byref(n32)) == 0  # the empty key
    # adl_bloom_revision_get: NULL revision, cache or num_hits; a key or a hit array that is missing
    fake = ctypes.c_void_p(p)  # never dereferenced: the checks come first
    args = (0, p, 2, 0, p, 4, ctypes.byref(n32), ctypes.byref(c32), ctypes.byref(u32), None)
    assert L.adl_bloom_revision_get(None, fake, *args) == INVALID_ARG
    assert L.adl_bloom_revision_get(rev._h, None, *args) == INVALID_ARG
    assert L.adl_bloom_revision_get(rev._h, fake, 0, p, 2, 0, p, 4, None, None, None, None) == INVALID_ARG
    assert L.adl_bloom_revision_get(rev._h, fake, 0, None, 2, 0, p, 4, ctypes.byref(n32), None, None,
                                    None) == INVALID_ARG
    assert L.adl_bloom_revision_get(rev._h, fake, 0, p, 2, 0, None, 4, ctypes.byref(n32), None, None,
                                    None) == INVALID_ARG
    # a level created without oids selects but cannot Get
    bare_lv = ab.LevelIndex(rk.tables("t3"))
    bare = ab.Revision([bare_lv])
    try:
        got, total = bare.candidates_host(b"ab")
        assert total == len(got)
        assert L.adl_bloom_revision_get(bare._h, fake, *args) == INVALID_ARG
        assert n32.value == 0 and c32.value == 0 and u32.value == 0  # (reset before the refusal)
    finally:
        bare.close()
        bare_lv.close()
    # adl_bloom_filter_cache_probe_key: NULL cache; tables without oids
    unc = ctypes.c_uint64(9)
    assert L.adl_bloom_filter_cache_probe_key(None, None, None, 0, 0, p, 2, p, ctypes.byref(unc), None) == INVALID_ARG
    assert L.adl_bloom_filter_cache_probe_key(fake, None, None, 3, 0, p, 2, p, ctypes.byref(unc), None) == INVALID_ARG


def _want(oracle, names, key, seq):
    return rk.revision_lists(oracle, names, [key], seq)[0]


def _keys(names):
    pool = rk.pool(names)
    # every boundary user key of every level is in the pool by construction; make sure of a few
    users = {bytes(t[i][:-9]) for n in names for t in rk.tables(n) for i in (0, 1)}
    assert len(users & set(pool)) >= 20
    rng = np.random.default_rng(0x17)
    short = [rng.integers(0x60, 0x68, L, dtype=np.uint8).tobytes() for L in range(18)]
    return pool + sorted(users - set(pool))[:40] + short


def test_candidates_host_vs_oracle(ab, oracle, five):
    names, rev = five
    keys = _keys(names)
    assert {len(k) for k in keys} >= set(range(18))
    differ, most = False, 0
    for seq in SEQS:
        for k in keys:
            want = _want(oracle, names, k, seq)
            got, total = rev.candidates_host(k, seq=seq)
            assert total == len(want) and list(got) == want, (seq, k, list(got), want)
            most = max(most, total)
            differ |= want != _want(oracle, names, k, 26)
    assert differ and most > 24  # the lists do differ by seq, and the 300-table level gives long ones
    base = rk.table_base(names)
    assert most >= 300 and int(base[-1]) == 319


def test_candidates_host_capacity(ab, oracle, five):
    names, rev = five
    keys = [k for k in _keys(names) if len(_want(oracle, names, k, 25)) >= 2][:60]
    assert len(keys) >= 30
    for k in keys:
        want = _want(oracle, names, k, 25)
        n = len(want)
        for cap in (n, n - 1, 0):
            tab = np.full(n + 2, 0xA5A5A5A5, np.uint32)
            num = ctypes.c_uint32()
            kb = np.frombuffer(k, np.uint8) if k else np.zeros(1, np.uint8)
            rc = ab.lib().adl_bloom_revision_candidates_host(rev._h, kb.ctypes.data, len(k), 25,
                                                             tab.ctypes.data if cap else None, cap, ctypes.byref(num))
            assert rc == 0 and num.value == n
            assert list(tab[:cap]) == want[:cap] and (tab[cap:] == 0xA5A5A5A5).all()


def test_empty_revision_has_no_candidates(ab):
    for levels in ([], [None, None]):
        rev = ab.Revision(levels)
        got, total = rev.candidates_host(b"anything")
        assert total == 0 and len(got) == 0
        rev.close()


# ------------------------------------------------------------------ the case table
@pytest.fixture(scope="module")
def g(oracle):
    return GK.load()


def test_case_table_expectations_are_the_oracles(g, oracle):
    n = 0
    for case in g.cases:
        for c in case.calls:
            want = g.expected(c)
            for i, t in enumerate(c.tables):
                tab = g.tables[t]
                if not g.resident(t):
                    assert want[i] == 1
                elif c.filter >= len(tab.bitmaps):
                    assert want[i] == 0
                else:
                    assert want[i] == int(oracle.probe([c.key], tab.bitmaps[c.filter], bits_per_key=tab.bpk)[0])
                n += 1
            assert c.path == ("server" if 1 <= len(c.tables) <= 24 and len(c.key) <= 96 else "launched")
    assert n > 1500


def test_case_table_covers_what_it_claims(g):
    cases = GK.by_name(g)
    # table counts: 1 .. 24 served, 25 launched; a member of all and a key none holds
    for n in GK.COUNTS:
        calls = cases["count-%d" % n].calls
        assert all(len(c.tables) == n for c in calls)
        assert [c.path for c in calls] == ["server" if n <= 24 else "launched"] * 3
        assert g.expected(calls[0]).all() and not g.expected(calls[1]).any() and g.expected(calls[2]).all()
    # exactly table j of 24, all, none
    for j in range(24):
        (c,) = cases["bit-%d" % j].calls
        assert len(c.tables) == 24 and c.path == "server"
        assert list(g.expected(c)) == [int(i == j) for i in range(24)]
    assert not g.expected(cases["bit-none"].calls[0]).any() and len(cases["bit-none"].calls[0].tables) == 24
    assert g.expected(cases["bit-all"].calls[0]).all() and len(cases["bit-all"].calls[0].tables) == 24
    # key lengths: 0 .. 96 served, 97 launched; both answers at every length; high bytes and the tail
    for L in GK.LENGTHS:
        calls = cases["len-%d" % L].calls
        assert all(len(c.key) == L for c in calls)
        assert all(c.path == ("server" if L <= 96 else "launched") for c in calls)
        answers = np.concatenate([g.expected(c) for c in calls])
        assert answers.any() and not answers.all(), L
        if L:
            assert min(calls[2].key) >= 0x80                               # every byte >= 0x80
            assert len(calls) == 6 and all(g.expected(c)[1] == 0 and g.expected(c)[3] == 0 for c in calls[4:])
        if L & 3:
            assert min(calls[3].key[L - (L & 3):]) >= 0x80 and max(calls[3].key[:L - (L & 3)], default=0) < 0x80
    # the mixed request: every k around kReads, every divisor class, an uncached and a removed table
    mixed = cases["mixed"].calls
    ks = {ab_k for c in mixed for ab_k in (SK.KS[t] for t in c.tables if t < SK.NT)}
    assert ks == {1, 5, 6, 7, 12, 13, 30}
    bits = {8 * len(g.tables[t].bitmaps[0]) for t in mixed[0].tables if g.resident(t)}
    assert {56, 128, 8192, 8184, 8200} <= bits
    assert all(g.uncached(c) == 2 and c.path == "server" for c in mixed)
    for t in (GK.M56, GK.M128, GK.M8192, SK.T_LO, SK.T_HI):
        col = [g.expected(c)[c.tables.index(t)] for c in mixed]
        assert (t == GK.M56) != any(col), t      # the empty filter answers 0 throughout, the others hold a key
        assert not all(col), t
    # no such filter: answers 0 from a resident block, 1 from an uncached table
    lack = cases["no-such-filter"].calls
    assert list(g.expected(lack[0])) == [1, 0, 0, 1, 0, 1] and list(g.expected(lack[1])) == [1, 0, 0, 1, 0, 1]
    assert list(g.expected(lack[2])) == [0, 0, 0, 1, 0, 0] and list(g.expected(lack[3])) == [0, 0, 0, 1, 0, 0]
