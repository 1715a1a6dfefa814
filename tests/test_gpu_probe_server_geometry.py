"""GPU: the resident probe server (adlsm-tree_amd/csrc/probe_server.hip) at
every request geometry of tests/serverkeys.py -- every key length 0..320 as a
member and as a non-member, requests that fill a slot to exactly 320 bytes and
keys at every offset mod 8 in it, the inline edge at 40/41 bytes, every k
around the groups of six bit reads, the divisor classes of the device-side
fastmod -- from an inline slot (0-3) and from slot 4 on purpose, with slots
shared by more threads than there are slots, with the kernel relaunched inside
the sweep, and across the wraps of the 24-bit answer tag and the 30-bit
sequence number (ADL_TEST_FAULT_SERVER_SEQ).

Every answer is compared exactly with the oracle under each table's own
bits_per_key (tests/test_probe_server_cases_cpu.py proves the expectations on
the CPU), and every call is repeated with ADL_BLOOM_PROBE_SERVER=0.  Which
path served a call is taken from adl_bloom_probe_server_phases' request count,
which counts served requests only: a call that fell back to a launched probe
(no answer within 200 ms) fails its case, and is not retried.

A thread's slot is the order in which threads first ask a cache's server
(probe_server.hip, probe: next_slot), so the tests never probe from the main
thread: they start short-lived threads one after another.
"""
import threading
import time

import numpy as np
import pytest

import serverkeys as SK

pytestmark = pytest.mark.gpu


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
def G(oracle):
    return SK.load()


def _cache(ab, G):
    """One mixed-bpk cache over every block of the table (and with it one server)."""
    cache = ab.FilterCache(4 << 20, max_tables=32)
    for t in G.tables:
        if t.block is not None:
            cache.put(t.oid, t.block)
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


def _ask(cache, G, c):
    keys, offs = SK.materialise(c)
    got, unc = cache.probe(G.oids, np.array(c.tables, np.uint32), keys, offs, filter=c.filter)
    return got.copy(), unc


def _touch(ab, cache, G):
    """One served single-key probe: the calling thread takes the server's next slot."""
    before = _served(ab)
    got, _ = _ask(cache, G, SK.call([G.member(16, 0)], [3]))
    assert got[0] == 1 and _served(ab) == before + 1, "the slot-taking probe was not served"


def _on_nth_thread(ab, cache, G, nth, fn):
    """fn() on the nth distinct thread to ask this cache's server: slot nth - 1."""
    for _ in range(nth - 1):
        _in_thread(lambda: _touch(ab, cache, G))
    return _in_thread(fn)


def _run_cases(ab, cache, G, cases, served, before_call=None):
    """Every call of the cases, exact against the oracle; per case the served
    count must have moved by the number of its calls the table marks "server"
    (served=False: the server is switched off, by none)."""
    answers, i = [], 0
    for case in cases:
        s0 = _served(ab)
        for j, c in enumerate(case.calls):
            if before_call:
                before_call(i)
            i += 1
            got, unc = _ask(cache, G, c)
            want = G.expected(c)
            assert np.array_equal(got, want), (case.name, j, "served" if served else "launched", got.tolist(),
                                               want.tolist())
            assert unc == G.uncached(c), (case.name, j)
            answers.append(got)
        want_served = sum(c.path == "server" for c in case.calls) if served else 0
        got_served = _served(ab) - s0
        assert got_served == want_served, (
            f"{case.name}: {got_served} of its calls were served by the resident kernel, {want_served} expected"
            " (a call fell back to a launched probe, or a launched one was served)")
    return answers


def _both_paths(ab, cache, G, knobs, cases, before_call=None):
    a = _run_cases(ab, cache, G, cases, True, before_call)
    knobs.set("ADL_BLOOM_PROBE_SERVER", "0")
    try:
        b = _run_cases(ab, cache, G, cases, False)
    finally:
        knobs.unset("ADL_BLOOM_PROBE_SERVER")
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    return len(a)


@pytest.mark.parametrize("nth", [1, 5], ids=["slot0-inline", "slot4"])
def test_every_geometry_vs_oracle(dev, ab, G, knobs, nth):
    """The whole case list from the first thread to ask the server (slot 0: its
    one-query requests of at most 40 key bytes go inline, the rest through the
    slot, so the bell's bit 31 flips from call to call) and from the fifth
    (slot 4: never inline)."""
    cache = _cache(ab, G)
    try:
        n = _on_nth_thread(ab, cache, G, nth, lambda: _both_paths(ab, cache, G, knobs, G.cases))
        assert n > 1700
    finally:
        cache.close()


def test_inline_edge_from_slots_1_to_3(dev, ab, G, knobs):
    """The other three inline slots (lines 1-3 of the wave's one line load):
    the keys around the 40/41-byte edge from the second, third and fourth thread."""
    by_name = {case.name: case for case in G.cases}
    cases = [by_name["len-%d" % L] for L in (0, 1, 39, 40, 41)] + [by_name["alt-40-41"]]
    cache = _cache(ab, G)
    try:
        _in_thread(lambda: _touch(ab, cache, G))  # slot 0
        for _ in (1, 2, 3):
            _in_thread(lambda: _both_paths(ab, cache, G, knobs, cases))
    finally:
        cache.close()


def test_slots_shared_by_more_threads_than_slots(dev, ab, G, knobs):
    """64 threads, one after another, take the server's 64 slots with one probe
    each; 8 more, running at once, then share slots 0-7 with the first eight
    (they continue those slots' sequence numbers and find their lines and done
    words as the earlier owners left them): 500 single-key probes each, keys
    of 16, 40, 41 and 200 bytes, members and non-members of the ten tables, every
    answer exact and every call served."""
    cache = _cache(ab, G)
    try:
        s0 = _served(ab)
        for _ in range(64):
            _in_thread(lambda: _touch(ab, cache, G))
        errors, asked = [], [set() for _ in range(8)]

        def worker(k):
            rng = np.random.default_rng(600 + k)
            for i in range(500):
                L = (16, 40, 41, 200)[int(rng.integers(0, 4))]
                t, kind = int(rng.integers(0, SK.NT)), int(rng.integers(0, 6))
                # (a member answers 1 in every one of the ten tables, G.non[t][L] answers 0 in table t:
                # tests/test_probe_server_cases_cpu.py, test_every_table_and_length_has_both_answers)
                key, want = (G.member(L, kind), 1) if kind < 4 else (G.non[t][L], 0)
                got, _ = _ask(cache, G, SK.call([key], [t]))
                if got[0] != want:
                    errors.append((k, i, L, t, kind, int(got[0])))
                asked[k].add((key, t, want))

        th = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors[:5]
        assert _served(ab) - s0 == 64 + 8 * 500, "a call fell back to a launched probe"
        knobs.set("ADL_BLOOM_PROBE_SERVER", "0")
        for key, t, want in sorted(set().union(*asked)):
            got, _ = _ask(cache, G, SK.call([key], [t]))
            assert got[0] == want, (len(key), t)
        assert _served(ab) - s0 == 64 + 8 * 500
    finally:
        knobs.unset("ADL_BLOOM_PROBE_SERVER")
        cache.close()


def test_relaunch_inside_the_sweep(dev, ab, G, knobs):
    """Keys of 30..50 bytes from slot 0 with a server that leaves after 100 us
    without a request, and 2 ms of sleep before every seventh call: a freshly
    started wave meets an inline request first, or a slot request."""
    knobs.set("ADL_BLOOM_SERVER_IDLE_US", "100")
    by_name = {case.name: case for case in G.cases}
    cases = [by_name["len-%d" % L] for L in range(30, 51)]
    cache = _cache(ab, G)
    try:
        l0 = ab.probe_server_launches()
        _in_thread(lambda: _both_paths(ab, cache, G, knobs, cases,
                                       lambda i: time.sleep(0.002) if i % 7 == 0 else None))
        moved = ab.probe_server_launches() - l0
        print("server kernels launched during the sweep:", moved)
        assert moved > 1, "the server kernel was never relaunched: the test proved nothing"
    finally:
        cache.close()


@pytest.mark.parametrize("relaunch", [False, True], ids=["resident", "relaunched"])
@pytest.mark.parametrize("preset", [(1 << 24) - 4, (1 << 30) - 4], ids=["tag-2^24", "seq-2^30"])
@pytest.mark.parametrize("nth", [1, 5], ids=["slot0-inline", "slot4"])
def test_sequence_wraps(dev, ab, G, knobs, nth, preset, relaunch):
    """12 requests across a wrap, the slot's sequence preset 4 below it
    (ADL_TEST_FAULT_SERVER_SEQ): the fourth request carries 2^24 (answer tag
    0x000000 after 0xFFFFFF) or, after 0x3FFFFFFF, sequence number 1 (0 is
    skipped).  40- and 41-byte keys in turn, a member and a non-member of each.
    resident: one kernel throughout (idle and life limits raised, at most the
    first kernel and its queued successor launched).  relaunched: the kernel
    leaves (idle 100 us, 2 ms of sleep) before the wrapping request and again
    after it, so the new wave takes its starting point from the done word
    written just before the wrap, and the next from the one written at it."""
    if relaunch:
        knobs.set("ADL_BLOOM_SERVER_IDLE_US", "100")
    else:
        knobs.set("ADL_BLOOM_SERVER_IDLE_US", "5000000")
        knobs.set("ADL_BLOOM_SERVER_LIFE_US", "600000000")
    calls = []
    for i in range(12):
        L, t = SK.INLINE + i % 2, (i + nth) % SK.NT
        calls.append(SK.call([G.member(L, i) if (i // 2) % 2 == 0 else G.non[t][L]], [t]))
    want = [1 if (i // 2) % 2 == 0 else 0 for i in range(12)]
    cache = _cache(ab, G)

    def body():
        s0, l0 = _served(ab), ab.probe_server_launches()
        l_wrap = None
        ab.test_fault(ab.TEST_FAULT_SERVER_SEQ, preset)
        try:
            for i, c in enumerate(calls):
                if relaunch and i in (3, 4):
                    if i == 3:
                        l_wrap = ab.probe_server_launches()
                    time.sleep(0.002)
                got, _ = _ask(cache, G, c)
                assert got[0] == want[i], (i, "served")
        finally:
            ab.test_fault(ab.TEST_FAULT_SERVER_SEQ, -1)
        assert _served(ab) - s0 == 12, "a request across the wrap was not served by the resident kernel"
        moved = ab.probe_server_launches() - l0
        if relaunch:
            assert ab.probe_server_launches() > l_wrap, "no kernel was launched at the wrap"
        elif nth == 1:
            assert 1 <= moved <= 2, "the first kernel and at most its queued successor"
        else:
            assert moved <= 1, "the kernel did not stay resident"
        knobs.set("ADL_BLOOM_PROBE_SERVER", "0")
        for i, c in enumerate(calls):
            got, _ = _ask(cache, G, c)
            assert got[0] == want[i], (i, "launched")
        assert _served(ab) - s0 == 12

    try:
        _on_nth_thread(ab, cache, G, nth, body)
    finally:
        knobs.unset("ADL_BLOOM_PROBE_SERVER")
        cache.close()
