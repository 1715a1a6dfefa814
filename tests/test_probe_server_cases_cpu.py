"""CPU: tests/serverkeys.py holds what it claims -- every request geometry of
the resident probe server with both expected answers, by the oracle alone.
tests/test_gpu_probe_server_geometry.py sends the same table to the server."""
import numpy as np
import pytest

import serverkeys as SK


@pytest.fixture(scope="module")
def G(oracle):
    return SK.load()


def _server_calls(G):
    return [(case.name, c) for case in G.cases for c in case.calls if c.path == "server"]


def test_member_set_has_four_keys_of_every_length_and_kind(G):
    assert len(G.members) == SK.MAXLEN + 1
    for L, four in enumerate(G.members):
        assert len(four) == 4 and all(len(k) == L for k in four)
        assert all(b >= 0x80 for b in four[2])
        r = L & 3
        assert all(b < 0x80 for b in four[3][:L - r]) and all(b >= 0x80 for b in four[3][L - r:])
        assert len(four[3][L - r:]) == r
    assert {L & 3 for L in range(SK.MAXLEN + 1)} == {0, 1, 2, 3}
    # the two random kinds are not accidentally of one sign: both signs occur in the long ones
    assert any(b >= 0x80 for b in G.members[64][0]) and any(b < 0x80 for b in G.members[64][0])


def test_tables_k_and_divisor_classes(G, oracle):
    assert [oracle.num_probes(b) for b in SK.BPKS] == list(SK.KS) == [1, 2, 5, 6, 7, 11, 12, 13, 29, 30]
    # the groups of six bit reads: below, at and above one, two and five groups
    assert {k % 6 for k in SK.KS} >= {0, 1, 5} and {-(-k // 6) for k in SK.KS} == {1, 2, 3, 5}
    n = len(G.flat)
    assert n == 4 * (SK.MAXLEN + 1)
    for t, bpk in enumerate(SK.BPKS):
        tab = G.tables[t]
        assert tab.bpk == bpk and len(tab.bitmaps) == 1
        assert tab.bitmaps[0].size == oracle.bitmap_bytes(n, bpk)
        rd = oracle.FilterBlockReaderOracle()
        assert rd.init(tab.block) == 0 and rd.bits_per_key == bpk and rd.filters_nums == 1
    multi = G.tables[SK.T_MULTI]
    assert multi.bpk == 9 and [len(m) for m in multi.members] == [0, 1, 113]
    assert [bm.size * 8 for bm in multi.bitmaps] == [56, 128, 1 << 13]
    assert [bm.size for bm in multi.bitmaps] == [oracle.bitmap_bytes(c, 9) for c in SK.MULTI_COUNTS]
    rd = oracle.FilterBlockReaderOracle()
    assert rd.init(multi.block) == 0 and rd.filters_nums == 3
    assert not multi.bitmaps[0].any()
    for t, m in ((SK.T_LO, (1 << 13) - 8), (SK.T_HI, (1 << 13) + 8)):
        tab = G.tables[t]
        assert tab.bpk == 1 and oracle.bitmap_bytes(len(tab.members[0]), 1) * 8 == m == tab.bitmaps[0].size * 8
    assert G.tables[SK.T_UNCACHED].block is None
    assert len(set(G.oids)) == len(G.oids) == SK.NT + 4


def test_every_table_and_length_has_both_answers(G, oracle):
    """The hard condition: for each of the ten tables and every length 1..320
    a key the oracle answers 1 (all four members) and one it answers 0.  The
    empty key is the only key of length 0 and a member of the ten: its 0 comes
    from the blocks that do not hold it."""
    for t, bpk in enumerate(SK.BPKS):
        bm = G.tables[t].bitmaps[0]
        assert oracle.probe(G.flat, bm, bits_per_key=bpk).all(), t
        non = G.non[t][1:]
        assert [len(k) for k in non] == list(range(1, SK.MAXLEN + 1))
        assert not oracle.probe(non, bm, bits_per_key=bpk).any(), t
    assert G.redraws[:, 0].sum() == 0 and G.redraws.max() < 200
    print("non-member redraws per table:", G.redraws.sum(axis=1).tolist(), "most for one key:", int(G.redraws.max()))
    zero = [c for case in G.cases if case.name == "len-0" for c in case.calls]
    want = [int(G.expected(c)[0]) for c in zero]
    assert 1 in want and 0 in want
    for c in zero:
        assert c.keys == (b"",)
    for key in G.universal:
        assert not any(oracle.probe([key], G.tables[t].bitmaps[0], bits_per_key=SK.BPKS[t])[0] for t in range(SK.NT))


def test_len_cases_cover_every_length_kind_and_answer(G):
    by_name = {case.name: case for case in G.cases}
    assert len(by_name) == len(G.cases)
    for L in range(SK.MAXLEN + 1):
        calls = by_name["len-%d" % L].calls
        assert all(len(c.keys) == 1 and len(c.keys[0]) == L and c.path == "server" for c in calls)
        assert {c.keys[0] for c in calls} >= set(G.members[L])
        want = {int(G.expected(c)[0]) for c in calls}
        assert want == {0, 1}, L
        if L:
            assert sum(c.keys[0] in G.members[L] for c in calls) == 4 and len(calls) == 6
    # both forms of a one-query request, at the inline edge and at the eligibility edge
    for L in (1, SK.INLINE, SK.INLINE + 1, SK.MAXLEN):
        assert {c.form for c in by_name["len-%d" % L].calls} == {"offsets", "stride"}
    # every table is asked for members and for non-members
    asked = {(c.tables[0], int(G.expected(c)[0])) for L in range(1, SK.MAXLEN + 1) for c in by_name["len-%d" % L].calls}
    assert asked == {(t, a) for t in range(SK.NT) for a in (0, 1)}


def test_pack_cases_fill_the_slot_exactly(G):
    by_name = {case.name: case for case in G.cases}
    starts, tails = set(), set()
    for n in range(2, SK.MAXQ + 1):
        second = set()
        for r in range(8):
            served, launched = by_name["pack-%d-%d" % (n, r)].calls
            assert len(served.keys) == len(launched.keys) == n
            assert served.nbytes == SK.MAXLEN and served.path == "server"
            assert launched.nbytes == SK.MAXLEN + 1 and launched.path == "launched"
            lens = [len(k) for k in served.keys]
            assert lens[0] == r
            off = np.concatenate([[0], np.cumsum(lens)])
            second.add(int(off[1]) % 8)
            starts |= {int(o) % 8 for o in off[:-1]}
            tails |= {L & 3 for L in lens}
            if n >= 4:
                assert lens[-1] == 0 and 0 in lens[1:-1]
            if n == 3:
                assert (lens[1] == 0) == (r % 2 == 0) and (lens[2] == 0) == (r % 2 == 1)
            assert len(set(served.tables)) > 1
            assert max(len(k) for c in (served, launched) for k in c.keys) <= SK.MAXLEN
        assert second == set(range(8)), n   # later keys start at every offset mod 8
    assert starts == set(range(8)) and tails == {0, 1, 2, 3}


def test_named_cases(G):
    by_name = {case.name: case for case in G.cases}
    for s in (1, 40, 41, 320):
        for c in by_name["stride-%d" % s].calls:
            assert c.form == "stride" and len(c.keys) == 1 and len(c.keys[0]) == s and c.path == "server"
        assert [int(G.expected(c)[0]) for c in by_name["stride-%d" % s].calls] == [1, 0]
    (c,) = by_name["stride-40x8"].calls
    assert c.form == "stride" and len(c.keys) == 8 and c.nbytes == 320 and c.path == "server"
    (c,) = by_name["stride-41x8"].calls
    assert c.form == "stride" and len(c.keys) == 8 and c.nbytes == 328 and c.path == "launched"
    for c in by_name["offs-base"].calls:
        data, offs = SK.materialise(c)
        assert c.form == "base" and int(offs[0]) == c.base > 0 and c.path == "server"
        assert [bytes(data[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])] == list(c.keys)
    assert any(c.base + c.nbytes > SK.MAXLEN for c in by_name["offs-base"].calls)
    for c in by_name["n9"].calls:
        assert len(c.keys) == 9 and all(len(k) == 16 for k in c.keys) and c.path == "launched"
    for name, want in (("alt-40-41", 1), ("alt-40-41-absent", 0)):
        calls = by_name[name].calls
        assert [len(c.keys[0]) for c in calls] == [40, 41] * 8
        assert all(len(c.keys) == 1 and c.path == "server" and int(G.expected(c)[0]) == want for c in calls)
    sweep = by_name["k-sweep"].calls
    assert [c.tables for c in sweep[:SK.NT]] == [(t,) * 8 for t in range(SK.NT)]
    assert len({c.keys for c in sweep}) == 1 and all(c.path == "server" for c in sweep)
    assert all(len(set(c.tables)) == 8 for c in sweep[SK.NT:])
    assert {t for c in sweep[SK.NT:] for t in c.tables} == set(range(SK.NT))
    for c in sweep:
        assert G.expected(c).tolist() == [1, 0] * 4
    assert {c.filter for case in G.cases for c in case.calls if SK.T_MULTI in c.tables} == {0, 1, 2, 3}
    for f in range(3):
        assert {int(a) for c in by_name["multi-f%d" % f].calls[1:] for a in G.expected(c)} == ({0, 1} if f else {0})
    for name in ("edge-1016", "edge-1018"):
        assert {int(G.expected(c)[0]) for c in by_name[name].calls} == {0, 1}
    assert any(G.uncached(c) for c in by_name["uncached"].calls)
    for c in by_name["uncached"].calls:
        assert all(a == 1 for a, t in zip(G.expected(c), c.tables) if t == SK.T_UNCACHED)
    for c in by_name["no-such-filter"].calls:
        assert c.filter >= 1
        for a, t in zip(G.expected(c), c.tables):
            if t < SK.NT or (t == SK.T_MULTI and c.filter == 3):
                assert a == 0
    assert 1700 < sum(len(case.calls) for case in G.cases) < 2600


def test_paths_follow_the_eligibility_rule(G):
    served = launched = 0
    sizes = set()
    for case in G.cases:
        for c in case.calls:
            data, offs = SK.materialise(c)
            n = len(c.keys)
            nbytes = int(offs[-1] - offs[0]) if offs is not None else data.shape[0] * data.shape[1]
            assert nbytes == c.nbytes
            assert c.path == ("server" if 1 <= n <= 8 and nbytes <= 320 else "launched"), case.name
            served += c.path == "server"
            launched += c.path == "launched"
            sizes.add(nbytes)
            assert all(0 <= t <= SK.T_UNCACHED for t in c.tables)
    assert {320, 321, 328} <= sizes and set(range(289, 321)) <= sizes
    assert served > 1700 and launched >= 7 * 8 + 3


def test_server_seq_preset_is_declared_and_accepted():
    """ADL_TEST_FAULT_SERVER_SEQ: additive (the ABI version stays), armed and
    disarmed without a device call; unknown sites are still refused."""
    import os

    import adlbloom

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "adl_bloom.h")).read()
    assert "#define ADL_TEST_FAULT_SERVER_SEQ 4\n" in header and "#define ADL_BLOOM_ABI_VERSION 1\n" in header
    assert adlbloom.TEST_FAULT_SERVER_SEQ == 4
    L = adlbloom.lib()
    assert L.adl_bloom_abi_version() == 1
    assert L.adl_bloom_test_fault(4, (1 << 30) - 4) == 0 and L.adl_bloom_test_fault(4, -1) == 0
    assert L.adl_bloom_test_fault(5, 0) == -1 and L.adl_bloom_test_fault(0, 0) == -1
    assert callable(adlbloom.probe_server_phases)


def test_expected_answers_recomputed_per_query(G, oracle):
    """Every expected answer again, one oracle.probe call per query under the
    table's own bits_per_key; every request of more than one query expects
    both answers."""
    checked = 0
    for case in G.cases:
        for c in case.calls:
            want = G.expected(c)
            for i, (k, t) in enumerate(zip(c.keys, c.tables)):
                tab = G.tables[t]
                if t == SK.T_UNCACHED:
                    again = 1
                elif c.filter >= len(tab.bitmaps):
                    again = 0
                else:
                    again = int(oracle.probe([k], tab.bitmaps[c.filter], bits_per_key=tab.bpk)[0])
                assert again == want[i], (case.name, i)
                checked += 1
            if len(c.keys) > 1:
                assert set(want.tolist()) == {0, 1}, case.name
    assert checked > 2500
