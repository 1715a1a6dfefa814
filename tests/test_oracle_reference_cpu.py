"""CPU: pin the oracle's bloom layer (oracle.keys2block, probe, filter_block_final,
FilterBlockReaderOracle) to the reference's compiled src/filter_block.cpp.

Every case is asserted against tests/golden/filter_block_ref.json, which
tests/golden/make_filter_block_ref.py recorded from
oracle/_ref/libref_filter_block.so (the reference's BloomFilter,
FilterBlockWriter and FilterBlockReader, unmodified), and, where that library
is built, against the library itself.  Every comparison is exact.  The cases
and their inputs are tests/refcases.py.
"""
import numpy as np
import pytest

import refcases as C


@pytest.fixture(scope="module")
def rec():
    return C.load_json()


@pytest.fixture(scope="module")
def ref(oracle):
    """The compiled reference, or None where oracle/_ref is not built (the JSON half stands alone)."""
    R = oracle.ref_filter_block_lib()
    return None if R is None else C.Ref(R)


def test_inputs_are_the_recorded_ones(oracle, rec):
    for shape, n in sorted({(s, n) for s, _, n in C.all_builds()}):
        assert C.members(shape, n).sha() == rec["inputs"][shape]["members"][str(n)]
        q = max(n, C.MIN_QUERIES)
        assert C.queries(shape, n).sha() == rec["inputs"][shape]["queries"][str(q)]
    # refcases' numpy SplitMix64 is the key stream of SURVEY.md §8d
    assert np.array_equal(C.members("split16", 1000).fixed(16), oracle.splitmix_keys16(0x5EED, 1000))
    assert np.array_equal(C.splitmix16(0x5EED, 10, skip=7).fixed(16), oracle.splitmix_keys16(0x5EED, 10, skip=7))
    assert (C.members("varlen", C.NMAX).data >= 0x80).mean() > 0.45
    lens = np.diff(C.members("varlen", C.NMAX).offs.astype(np.int64))
    assert lens.min() == 0 and lens.max() == 69


def test_grid_is_the_recorded_one(rec):
    assert set(rec["builds"]) == {C.build_id(*c) for c in C.all_builds()}
    assert set(rec["blocks"]) == set(C.BLOCKS)
    assert set(rec["mutations"]["cases"]) == set(MUTATION_NAMES)


def _dummy_trailer():
    """A 3-filter trailer over a 33-byte body, only to enumerate the mutations' names."""
    import struct

    body = 33
    return struct.pack("<5i", 0, 11, 22, body, 3) + b"bf:" + struct.pack("<2i", 10, 7)


@pytest.mark.parametrize("shape,bpk,n", C.all_builds())
def test_keys2block_and_probe(oracle, rec, ref, shape, bpk, n):
    g = rec["builds"][C.build_id(shape, bpk, n)]
    k = C.members(shape, n)
    bm = oracle.keys2block(k.data, k.offs, bits_per_key=bpk)
    assert bm.size == g["bytes"] == n * bpk + 7
    assert C.sha(bm) == g["sha256"]
    if shape in ("split16", "fixed24"):  # the oracle's fixed-stride form of the same keys
        assert np.array_equal(oracle.keys2block(k.fixed(int(shape[-2:])), bits_per_key=bpk), bm)
    if ref is not None:
        assert ref.keys2block(bpk, k) == bm.tobytes()
    if n == 0:
        assert "q_bits" not in g and "q_sha256" not in g
        return
    got_m = oracle.probe(k.data, bm, offsets=k.offs, bits_per_key=bpk)
    assert got_m.all()  # every member answers 1
    q = C.queries(shape, n)
    got = oracle.probe(q.data, bm, offsets=q.offs, bits_per_key=bpk)
    assert set(np.unique(got)) <= {0, 1}
    if "q_bits" in g:
        assert q.n == C.MIN_QUERIES and C.bits_hex(got) == g["q_bits"]
    else:
        assert q.n == n and int(got.sum()) == g["q_ones"]
        assert C.sha(got.tobytes()) == g["q_sha256"]
    if ref is not None:
        assert np.array_equal(ref.probe(bpk, k, bm.tobytes()), got_m)
        assert np.array_equal(ref.probe(bpk, q, bm.tobytes()), got)
        # the single-key entry point of the harness, on a few
        for i in range(0, q.n, max(q.n // 7, 1)):
            key = q.key(i)
            assert ref.R.ref_is_key_exists(bpk, key, len(key), bm.ctypes.data, bm.size) == got[i]


def _oracle_block(oracle, name):
    shape, bpk, counts = C.BLOCKS[name]
    k = C.block_keys(name)
    kb = np.concatenate([[0], np.cumsum(counts)])
    bms = []
    for f in range(len(counts)):
        s = k.slice(int(kb[f]), int(kb[f + 1]))
        bms.append(oracle.keys2block(s.data, s.offs, bits_per_key=bpk).tobytes())
    return oracle.filter_block_final(bms, bpk)


@pytest.mark.parametrize("name", list(C.BLOCKS))
def test_filter_block_final_and_reader(oracle, rec, ref, name):
    g = rec["blocks"][name]
    shape, bpk, counts = C.BLOCKS[name]
    F = len(counts)
    assert C.block_keys(name).sha() == g["keys_sha256"]
    blk = _oracle_block(oracle, name)
    assert len(blk) == g["bytes"]
    assert C.sha(blk) == g["sha256"]
    assert [[len(b), C.sha(b)] for b in C.split_block(blk)[0]] == g["bitmaps"]
    ids, q = C.block_queries(name)
    assert C.sha(ids.astype("<i4").tobytes() + bytes.fromhex(q.sha())) == g["queries_sha256"]
    assert set(ids.tolist()) == set(range(F + 2))
    rd = oracle.FilterBlockReaderOracle()
    assert rd.init(blk) == 0 and rd.filters_nums == F and rd.bits_per_key == bpk
    got = np.array([rd.is_key_exists(int(ids[i]), q.key(i)) for i in range(q.n)], dtype=np.uint8)
    assert C.bits_hex(got) == g["answers"]
    assert not got[ids >= F].any()
    if ref is not None:
        assert ref.block(bpk, C.block_keys(name), counts) == blk
        assert ref.reader_init(blk) == 0
        assert np.array_equal(ref.reader_probe(blk, ids, q), got.astype(np.int8))
        for i in range(0, q.n, max(q.n // 11, 1)):
            assert ref.reader_exists(blk, int(ids[i]), q.key(i)) == got[i]


def test_block_cases_cover_what_they_should():
    F = {name: len(c) for name, (_, _, c) in C.BLOCKS.items()}
    assert 1 in F.values() and 70 in F.values()
    assert {b for _, b, _ in C.BLOCKS.values()} >= {1, 10, 44}
    e = C.EMPTIES
    assert e[0] == 0 and e[-1] == 0 and any(a == b == 0 for a, b in zip(e, e[1:])) and any(e)
    assert sum(c == 0 for c in C.C70) == 8 and C.C70[0] == 0


# Trailer mutations the oracle (like adlsm-tree_amd/csrc/filter_block_format.hpp, which it restates)
# rejects although the reference's Init accepts them, each with the reason given there.  In every one
# the reference's IsKeyExists then reads outside the block or outside the filter it was asked about.
REJECTED_THOUGH_REFERENCE_ACCEPTS = {
    "F=-1": "a negative filter count: nf < 0 is refused (the reference answers 0 for every id)",
    "F=1000": "the offsets array must lie inside the block, before the count field; the reference's "
              "IsKeyExists reads its entries beyond the block",
    "off_1>off_2": "offsets out of order: the reference forms a bitmap of negative length and reads outside it",
    "off_2>offsets_start": "an offset beyond offsets_start: the last filter's range would have negative length",
}
# Accepted by both, but one filter id is an empty range, for which the reference computes h % 0
# (src/filter_block.cpp:56); the oracle and the product answer 0 (adlsm-tree_amd/csrc/probe_device.hpp).
EMPTY_RANGE_ANSWERS_0 = {
    "F=4": "filter 3's offset is the offsets_start field itself, so filter 3 is [offsets_start, offsets_start)",
}


@pytest.fixture(scope="module")
def base3(oracle, rec):
    k, counts = C.base3()
    kb = np.concatenate([[0], np.cumsum(counts)])
    bms = []
    for f in range(3):
        s = k.slice(int(kb[f]), int(kb[f + 1]))
        bms.append(oracle.keys2block(s.data, s.offs, bits_per_key=C.BASE3_BPK).tobytes())
    blk = oracle.filter_block_final(bms, C.BASE3_BPK)
    g = rec["mutations"]["base"]
    assert len(blk) == g["bytes"] and C.sha(blk) == g["sha256"]
    # filters 0 and 1 are the block of the reference's test/filter_block_test.cpp
    assert blk[:sum(len(b) for b in bms[:2])] == bms[0] + bms[1] and len(bms[0]) == 100047
    assert rec["mutations"]["ids"] == list(C.MUT_IDS) and rec["mutations"]["keys"] == [k.hex() for k in C.MUT_KEYS]
    return blk, C.mutations(blk)


MUTATION_NAMES = sorted(C.mutations(bytes(33) + _dummy_trailer()))


@pytest.mark.parametrize("name", MUTATION_NAMES)
def test_reader_trailer_mutation(oracle, rec, ref, base3, name):
    blk = base3[1][name]
    rd = oracle.FilterBlockReaderOracle()
    got_rc = rd.init(blk)
    C.check_reader_rule(name, rec["mutations"]["cases"][name], got_rc, rd.is_key_exists,
                        REJECTED_THOUGH_REFERENCE_ACCEPTS, EMPTY_RANGE_ANSWERS_0)
    if ref is not None:
        rc, ans = ref.mutation(blk)
        assert {"rc": rc, "answers": ans} == rec["mutations"]["cases"][name]


def test_reader_divergences_are_exactly_the_listed_ones(oracle, rec, base3):
    rejected, empty = set(), set()
    for name, blk in base3[1].items():
        g = rec["mutations"]["cases"][name]
        if g["rc"] == 0 and oracle.FilterBlockReaderOracle().init(blk) != 0:
            rejected.add(name)
        if g["rc"] == 0 and "z" in g["answers"]:
            empty.add(name)
    assert rejected == set(REJECTED_THOUGH_REFERENCE_ACCEPTS)
    assert empty == set(EMPTY_RANGE_ANSWERS_0)
    # the well-formed block is among the mutations (info_len = 7, F = 3) and is accepted
    assert base3[1]["info_len=7"] == base3[0] == base3[1]["F=3"]
    assert rec["mutations"]["cases"]["F=3"]["rc"] == 0
