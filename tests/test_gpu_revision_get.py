"""GPU: the single-key revision Get -- one key, all its candidate tables, ONE
request to the resident probe server (the fan form of a slot,
adlsm-tree_amd/csrc/probe_server.hip) -- through FilterCache.probe_key and
Revision.get.

Every answer is compared exactly with the oracle (tests/getkeys.py, which
tests/test_revision_get_cpu.py proves on the CPU) and with the same call under
ADL_BLOOM_PROBE_SERVER=0.  Which path served a call is taken from
adl_bloom_probe_server_phases' request count, which must move by exactly one
per call the table marks "server" and by none otherwise, and from
adl_bloom_probe_server_launches, which must not move on a served call: a call
that fell back to a launched probe (no answer within 200 ms) fails its case,
and is not retried.  The table-driven tests keep one kernel resident (idle and
life limits raised) and start once it and its queued successor are launched.

A thread's slot is the order in which threads first ask a cache's server, so
the tests never probe from the main thread: they start short-lived threads one
after another (as tests/test_gpu_probe_server_geometry.py does).
"""
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import getkeys as GK
import revisionkeys as rk
import serverkeys as SK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.fixture(scope="module")
def g(oracle):
    return GK.load()


def _cache(ab, g):
    """One mixed-bpk cache over every block of the table (and with it one server)."""
    cache = ab.FilterCache(8 << 20, max_tables=64)
    cache.launches_before = ab.probe_server_launches()
    for t in g.tables:
        if t.block is not None:
            cache.put(t.oid, t.block)
    assert cache.remove(g.oids[GK.REMOVED])
    return cache


def _in_thread(fn):
    """fn() on a fresh thread, joined; what it raised is raised here."""
    box = []

    def run():
        try:
            box.append((True, fn()))
        except BaseException as e:  # noqa: BLE001 (re-raised below)
            box.append((False, e))

    t = threading.Thread(target=run)
    t.start()
    t.join()
    ok, v = box[0]
    if not ok:
        raise v
    return v


def _served(ab):
    return ab.probe_server_phases()[0]


def _ask(cache, g, c):
    """An ordinary request (a tests/serverkeys.py call: a key per query)."""
    keys, offs = SK.materialise(c)
    got, unc = cache.probe(g.oids, np.array(c.tables, np.uint32), keys, offs, filter=c.filter)
    return got.copy(), unc


def _get(cache, g, c):
    """A Get (a tests/getkeys.py call: one key, its tables)."""
    got, unc = cache.probe_key([g.oids[t] for t in c.tables], c.key, filter=c.filter)
    return got.copy(), unc


def _touch(ab, cache, g):
    """One served single-key probe: the calling thread takes the server's next slot."""
    before = _served(ab)
    got, _ = _ask(cache, g, SK.call([g.G.member(16, 0)], [3]))
    assert got[0] == 1 and _served(ab) == before + 1, "the slot-taking probe was not served"


def _settle(ab, cache, ask):
    """ask() -- a served request -- until the cache's server has launched its
    first kernel and the successor that the launcher thread queues behind it,
    off the request path: with the idle and life limits raised nothing is
    launched after that."""
    for _ in range(200000):
        ask()
        if ab.probe_server_launches() >= cache.launches_before + 2:
            return
    raise AssertionError("the server's successor kernel was never queued")


def _on_nth_thread(ab, cache, g, nth, fn):
    """fn() on the nth distinct thread to ask this cache's server: slot nth - 1."""
    for _ in range(nth - 1):
        _in_thread(lambda: _touch(ab, cache, g))
    return _in_thread(fn)


def _resident(knobs):
    knobs.set("ADL_BLOOM_SERVER_IDLE_US", "5000000")
    knobs.set("ADL_BLOOM_SERVER_LIFE_US", "600000000")


def _check_get(ab, cache, g, c, served, where):
    s0, l0 = _served(ab), ab.probe_server_launches()
    got, unc = _get(cache, g, c)
    moved, launched = _served(ab) - s0, ab.probe_server_launches() - l0
    want = g.expected(c)
    assert np.array_equal(got, want), (where, "served" if served else "launched", got.tolist(), want.tolist())
    assert unc == g.uncached(c), where
    want_moved = 1 if served and c.path == "server" else 0
    assert moved == want_moved, (
        f"{where}: the served-request count moved by {moved}, {want_moved} expected (a Get fell back to a launched "
        "probe, took more than one request, or a launched one was served)")
    if want_moved:
        assert launched == 0, f"{where}: a server kernel was launched during a served Get"
    return got


def _run_cases(ab, cache, g, cases, served):
    return [_check_get(ab, cache, g, c, served, (case.name, j)) for case in cases for j, c in enumerate(case.calls)]


def _both_paths(ab, cache, g, knobs, cases):
    _settle(ab, cache, lambda: _touch(ab, cache, g))
    a = _run_cases(ab, cache, g, cases, True)
    knobs.set("ADL_BLOOM_PROBE_SERVER", "0")
    try:
        b = _run_cases(ab, cache, g, cases, False)
    finally:
        knobs.unset("ADL_BLOOM_PROBE_SERVER")
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    return len(a)


@pytest.mark.parametrize("nth", [1, 5], ids=["slot0-inline", "slot4"])
def test_every_get_vs_oracle(dev, ab, g, knobs, nth):
    """The whole case list -- 1 .. 25 tables, "exactly table j of 24", key
    lengths 0 .. 97, the request of mixed k and filter sizes with an uncached
    and a removed table, filters the blocks lack -- from slot 0 and from slot 4."""
    _resident(knobs)
    cache = _cache(ab, g)
    try:
        n = _on_nth_thread(ab, cache, g, nth, lambda: _both_paths(ab, cache, g, knobs, g.cases))
        assert n > 150
    finally:
        cache.close()


@pytest.mark.parametrize("nth", [1, 5], ids=["slot0-inline", "slot4"])
def test_form_changes_on_one_slot(dev, ab, g, knobs, nth):
    """Fan, a one-key Get (inline on slot 0), an 8-query slot request, fan
    again, over and over on one slot with the same answers each time: the fan
    requests' extra answer words stay behind while the other forms are served,
    and must never pair with a later request's tag."""
    _resident(knobs)
    cases = GK.by_name(g)
    sk = {case.name: case for case in g.G.cases}
    inline = SK.call([g.G.member(16, 1)], [3])
    absent = SK.call([g.G.non[4][40]], [4])
    eight = sk["k-sweep"].calls[SK.NT]  # 8 keys, tables 0 .. 7
    assert len(eight.keys) == 8 and eight.path == "server" and inline.path == "server"
    cache = _cache(ab, g)

    def body():
        _settle(ab, cache, lambda: _touch(ab, cache, g))
        n = 0
        for r in range(8):
            fans = [cases["bit-%d" % ((5 * r + 17) % 24)].calls[0], cases["bit-all" if r % 2 else "bit-none"].calls[0],
                    cases["count-%d" % GK.COUNTS[r % 9]].calls[r % 2], cases["mixed"].calls[r % 7]]
            for i, fan in enumerate(fans):
                _check_get(ab, cache, g, fan, True, ("fan", r, i))
                for c in (inline, eight, absent)[:1 + (r + i) % 3]:
                    s0 = _served(ab)
                    got, _ = _ask(cache, g, c)
                    assert np.array_equal(got, g.G.expected(c)) if c is eight else got[0] == (c is inline), (r, i)
                    assert _served(ab) == s0 + 1, "an ordinary request between two fan requests was not served"
                    n += 1
                _check_get(ab, cache, g, fan, True, ("fan again", r, i))
        return n

    try:
        assert _on_nth_thread(ab, cache, g, nth, body) >= 48
    finally:
        cache.close()


@pytest.mark.parametrize("relaunch", [False, True], ids=["resident", "relaunched"])
@pytest.mark.parametrize("preset", [(1 << 24) - 4, (1 << 30) - 4], ids=["tag-2^24", "seq-2^30"])
def test_sequence_wraps_on_fan_requests(dev, ab, g, knobs, preset, relaunch):
    """12 fan requests of 24 tables across a wrap, the slot's sequence preset 4
    below it (ADL_TEST_FAULT_SERVER_SEQ): the fourth request carries 2^24
    (answer tag 0x000000 after 0xFFFFFF, in all three tagged words) or, after
    0x3FFFFFFF, sequence number 1.  resident: one kernel throughout.
    relaunched: the kernel leaves (idle 100 us, 2 ms of sleep) before the
    wrapping request and again after it, so the new wave takes its starting
    point from the done word written just before the wrap, and the next from
    the one written at it."""
    if relaunch:
        knobs.set("ADL_BLOOM_SERVER_IDLE_US", "100")
    else:
        _resident(knobs)
    cases = GK.by_name(g)
    calls = [cases["bit-%d" % ((7 * i + 3) % 24)].calls[0] if i % 3 else cases["bit-all" if i % 2 else "bit-none"].calls[0]
             for i in range(12)]
    cache = _cache(ab, g)

    def body():
        if not relaunch:
            _settle(ab, cache, lambda: _touch(ab, cache, g))
        s0, l0 = _served(ab), ab.probe_server_launches()
        l_wrap = None
        ab.test_fault(ab.TEST_FAULT_SERVER_SEQ, preset)
        try:
            for i, c in enumerate(calls):
                if relaunch and i in (3, 4):
                    if i == 3:
                        l_wrap = ab.probe_server_launches()
                    time.sleep(0.002)
                got, _ = _get(cache, g, c)
                assert np.array_equal(got, g.expected(c)), (i, "served", got.tolist())
        finally:
            ab.test_fault(ab.TEST_FAULT_SERVER_SEQ, -1)
        assert _served(ab) - s0 == 12, "a fan request across the wrap was not served by the resident kernel"
        if relaunch:
            assert ab.probe_server_launches() > l_wrap, "no kernel was launched at the wrap"
        else:
            assert ab.probe_server_launches() == l0, "the kernel did not stay resident"
        knobs.set("ADL_BLOOM_PROBE_SERVER", "0")
        for i, c in enumerate(calls):
            got, _ = _get(cache, g, c)
            assert np.array_equal(got, g.expected(c)), (i, "launched")
        assert _served(ab) - s0 == 12

    try:
        _in_thread(body)
    finally:
        knobs.unset("ADL_BLOOM_PROBE_SERVER")
        cache.close()


def test_72_threads_alternate_fan_and_ordinary_requests(dev, ab, g, knobs):
    """64 threads, one after another, take the server's 64 slots with a fan and
    an ordinary request each; 8 more, running at once, then share slots 0-7
    with the first eight: 150 fan and 150 ordinary requests each, in turn,
    every answer exact and every call served."""
    cases = GK.by_name(g)
    fans = [c for name in ["bit-%d" % j for j in range(24)] + ["bit-all", "bit-none", "mixed", "count-9", "count-17",
                                                                "len-95", "len-96", "len-0"]
            for c in cases[name].calls]
    assert all(c.path == "server" for c in fans)
    cache = _cache(ab, g)
    try:
        s0 = _served(ab)

        def first(i):
            _touch(ab, cache, g)
            c = fans[i % len(fans)]
            got, _ = _get(cache, g, c)
            assert np.array_equal(got, g.expected(c)), i

        for i in range(64):
            _in_thread(lambda: first(i))
        errors = []

        def worker(k):
            rng = np.random.default_rng(900 + k)
            for i in range(150):
                c = fans[int(rng.integers(0, len(fans)))]
                got, unc = _get(cache, g, c)
                if not np.array_equal(got, g.expected(c)) or unc != g.uncached(c):
                    errors.append((k, i, "fan", got.tolist()))
                L = (16, 40, 41, 200)[int(rng.integers(0, 4))]
                t, member = int(rng.integers(0, SK.NT)), bool(rng.integers(0, 2))
                got, _ = _ask(cache, g, SK.call([g.G.member(L, i) if member else g.G.non[t][L]], [t]))
                if got[0] != member:
                    errors.append((k, i, "ordinary", L, t, int(got[0])))

        th = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors[:5]
        assert _served(ab) - s0 == 64 * 2 + 8 * 300, "a call fell back to a launched probe"
    finally:
        cache.close()


# ------------------------------------------------------------------ Revision.get
def _five(ab, oracle):
    """The five-level revision of tests/revisionkeys.py (t3, an empty level, a
    missing one, t16 and the 300 nested tables), every table with a filter
    block of its own -- bits_per_key 3, 10 and 44 in turn over every third pool
    key -- in one cache; table 7 is never cached and table 11 removed again."""
    names = rk.REVISIONS["five"]
    pool = rk.pool(names)
    rng = np.random.default_rng(0x6E7)
    keys = [pool[int(i)] for i in rng.permutation(len(pool))[:200]]
    base = rk.table_base(names)
    T = int(base[-1])
    bpk = [(3, 10, 44)[t % 3] for t in range(T)]
    oids = [b"get5-%d" % t for t in range(T)]
    cache = ab.FilterCache(16 << 20, max_tables=512)
    cache.launches_before = ab.probe_server_launches()
    truth = []
    for t in range(T):
        bm = oracle.keys2block([k for i, k in enumerate(pool) if (i + t) % 3 == 0], bits_per_key=bpk[t])
        truth.append(oracle.probe(keys, bm, bits_per_key=bpk[t]))
        if t != 7:
            cache.put(oids[t], oracle.filter_block_final([bm.tobytes()], bpk[t]))
    assert cache.remove(oids[11])
    cached = [t not in (7, 11) for t in range(T)]
    levels = []
    for l, n in enumerate(names):
        lo, hi = int(base[l]), int(base[l + 1])
        levels.append(None if n is None else ab.LevelIndex(rk.tables(n), oids=oids[lo:hi]))
    return names, keys, truth, cached, oids, cache, levels, ab.Revision(levels)


def test_revision_get_on_five_cached_levels(dev, ab, oracle, knobs):
    _resident(knobs)
    names, keys, truth, cached, oids, cache, levels, rev = _five(ab, oracle)
    data, offs = oracle.pack(keys)

    def body():
        # (the multi-gets first: their device copies and staging are made while no server kernel is resident)
        multi = {seq: rev.multiget(cache, data, offs, seq=seq) for seq in (25, SEQ_MAX)}
        easy = next(k for k, cand in zip(keys, rk.revision_lists(oracle, names, keys, SEQ_MAX))
                    if 1 <= len(cand) <= 24 and len(k) <= 96)
        _settle(ab, cache, lambda: rev.get(cache, easy))
        served = launched = hits = misses = 0
        for seq in (25, SEQ_MAX):
            lists = rk.revision_lists(oracle, names, keys, seq)
            hb, ht, _ = multi[seq]
            for i, (k, cand) in enumerate(zip(keys, lists)):
                want = [t for t in cand if not cached[t] or truth[t][i]]
                want_unc = sum(not cached[t] for t in want)
                fits = 1 <= len(cand) <= 24 and len(k) <= 96
                s0, l0 = _served(ab), ab.probe_server_launches()
                rc, got, nh, nc, unc = rev.get_status(cache, k, seq=seq)
                moved, relaunched = _served(ab) - s0, ab.probe_server_launches() - l0
                assert rc == 0 and nc == len(cand) and nh == len(want), (seq, i, k, rc, nc, nh)
                assert list(got) == want and unc == want_unc, (seq, i, k, list(got), want)
                assert list(got) == list(ht[int(hb[i]):int(hb[i + 1])]), (seq, i, "differs from multiget's list")
                assert moved == int(fits), (seq, i, len(cand), len(k), moved)
                assert not (fits and relaunched), (seq, i, "a server kernel was launched during a served Get")
                served += fits
                launched += len(cand) > 24
                hits += len(want)
                misses += len(cand) - len(want)
                # hit_capacity one short: ADL_ERR_WORKSPACE, the count reported, nothing written
                if want and i % 5 == 0:
                    rc, short, nh2, nc2, _ = rev.get_status(cache, k, seq=seq, hit_capacity=len(want) - 1)
                    assert rc == ab.ADL_ERR_WORKSPACE and nh2 == len(want) and nc2 == len(cand)
                    assert (short == 0xA5A5A5A5).all()
        # (what the pool exercises: Gets within one server request and beyond it, hits and filtered tables)
        assert served > 50 and launched > 5 and hits > 200 and misses > 200
        # the launched path gives the same lists
        knobs.set("ADL_BLOOM_PROBE_SERVER", "0")
        s0 = _served(ab)
        lists = rk.revision_lists(oracle, names, keys, SEQ_MAX)
        for i, (k, cand) in enumerate(zip(keys, lists)):
            got, _ = rev.get(cache, k)
            assert list(got) == [t for t in cand if not cached[t] or truth[t][i]], (i, "launched")
        assert _served(ab) == s0

    try:
        _in_thread(body)
        # every pin was given back, the short-capacity calls' included: removed, the ranges are free at once
        knobs.unset("ADL_BLOOM_PROBE_SERVER")
        assert all(cache.remove(o) for t, o in enumerate(oids) if cached[t])
        assert cache.stats() == (0, 0)
    finally:
        knobs.unset("ADL_BLOOM_PROBE_SERVER")
        cache.close()  # (first: it stops the resident kernel, which the frees below would wait for)
        rev.close()
        for lv in levels:
            if lv is not None:
                lv.close()


def test_revision_get_binary(dev):
    """bin/revision_get_test: RevisionGetFilter equals the one-key
    RevisionMultiGetFilter key by key, four threads, five levels with an empty
    and a missing one, Gets within one server request and beyond it."""
    exe = os.path.join(ROOT, "adlsm-tree_amd", "bin", "revision_get_test")
    assert os.path.exists(exe), f"{exe} is missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items()
           if k not in ("ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS", "ADL_BLOOM_REVISION_DEVICE_MIN_KEYS")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
