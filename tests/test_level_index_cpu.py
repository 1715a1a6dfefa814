"""CPU: the resident level index (adl_bloom_level, level_index_core.hpp; the
C++ LevelIndex in adlsm-tree_amd/csrc/level_filter.cpp) -- ONE index built per
level answers batches at several sequence numbers from its host copy, and each
answer equals the oracle's restatement of src/revision.cpp:278-287
(oracle.level_candidates) and LevelCandidates called fresh for that batch.
Host code only: no compute call reaches the GPU (the device copy of an index
is made by its first device call)."""
import ctypes
import os
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "adlsm-tree_amd", "lib", "libadlfilterblock.so")
PP = ctypes.POINTER(ctypes.c_char_p)


@pytest.fixture(scope="module")
def mirror():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} is missing: run __graft_entry__.build()")
    L = ctypes.CDLL(LIB)
    f = L.adl_level_candidates
    f.restype = ctypes.c_int64
    f.argtypes = [PP, ctypes.c_void_p, PP, ctypes.c_void_p, ctypes.c_uint32, PP, ctypes.c_void_p, ctypes.c_uint32,
                  ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    g = L.adl_level_index_candidates
    g.restype = ctypes.c_int64
    g.argtypes = [PP, ctypes.c_void_p, PP, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, PP, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_uint64]
    return f, g


def inner(user: bytes, seq: int, op: int) -> bytes:
    return user + struct.pack("<q", seq) + bytes([op])


def _arr(bs):
    return (ctypes.c_char_p * max(len(bs), 1))(*bs), np.array([len(b) for b in bs] or [0], dtype=np.uint64)


def fresh_candidates(f, tables, keys, seq):
    """adl_level_candidates: LevelCandidates, the index rebuilt for this batch."""
    mins, ml = _arr([t[0] for t in tables])
    maxs, xl = _arr([t[1] for t in tables])
    ks, kl = _arr(keys)
    cap = len(tables) * len(keys) + 1
    begin = np.zeros(len(keys) + 1, dtype=np.uint32)
    table = np.zeros(cap, dtype=np.uint32)
    n = f(mins, ml.ctypes.data, maxs, xl.ctypes.data, len(tables), ks, kl.ctypes.data, len(keys), seq,
          begin.ctypes.data, table.ctypes.data, cap)
    assert n >= 0
    return [list(table[begin[i]:begin[i + 1]]) for i in range(len(keys))]


def index_candidates(g, tables, batches, max_index_bytes=0):
    """adl_level_index_candidates: one LevelIndex, then every (keys, seq) batch
    from its host copy.  -> per batch, per key, the list of tables."""
    mins, ml = _arr([t[0] for t in tables])
    maxs, xl = _arr([t[1] for t in tables])
    allkeys = [k for keys, _ in batches for k in keys]
    ks, kl = _arr(allkeys)
    kb = np.concatenate([[0], np.cumsum([len(keys) for keys, _ in batches])]).astype(np.uint32)
    seqs = np.array([s for _, s in batches], dtype=np.int64)
    cap = len(tables) * len(allkeys) + 1
    begin = np.zeros(len(allkeys) + len(batches), dtype=np.uint32)
    table = np.zeros(cap, dtype=np.uint32)
    n = g(mins, ml.ctypes.data, maxs, xl.ctypes.data, len(tables), max_index_bytes, ks, kl.ctypes.data,
          kb.ctypes.data, len(batches), seqs.ctypes.data, begin.ctypes.data, table.ctypes.data, cap)
    assert n >= 0, n
    out, base = [], 0
    for b, (keys, _) in enumerate(batches):
        bg = begin[int(kb[b]) + b:int(kb[b + 1]) + b + 1]
        assert bg[0] == 0
        out.append([list(table[base + bg[i]:base + bg[i + 1]]) for i in range(len(keys))])
        base += int(bg[-1])
    assert base == n
    return out


def random_level(oracle, rng):
    """A level of test_level_cpu.py's kind: overlapping ranges over few user
    keys, equal minimums, a repeated range, inner keys shorter than 9 bytes
    and a table whose max sorts before its min.  Max seqs are drawn from
    {24, 25, 26} with op 0 or 1, so the batches at seq 25 meet tables below,
    at (op 0 and op > 0) and above it."""
    users = sorted({bytes(rng.integers(97, 101, int(rng.integers(1, 4))).astype(np.uint8)) for _ in range(30)})
    T = int(rng.integers(6, 40))
    tables = []
    for _ in range(T):
        a, b = sorted(rng.integers(0, len(users), 2))
        s1, s2 = int(rng.integers(0, 50)), int(rng.integers(24, 27))
        mn, mx = inner(users[a], s1, int(rng.integers(0, 2))), inner(users[b], s2, int(rng.integers(0, 2)))
        if a == b and oracle._memkey_less(oracle._decode_inner(mx), oracle._decode_inner(mn)):
            mn, mx = mx, mn
        tables.append((mn, mx))
    tables[1] = (tables[0][0], tables[1][1])  # equal min keys
    tables[3] = tables[2]                     # a range repeated
    tables[4] = (users[1], users[-2])         # shorter than 9 bytes: (user, seq 0, op 0)
    tables[5] = (inner(users[-1], 5, 0), inner(users[0], 25, 1))  # max < min: never a candidate
    return users, tables


@pytest.mark.parametrize("seed", range(24))
def test_one_index_answers_batches_at_several_seqs(mirror, oracle, seed):
    f, g = mirror
    rng = np.random.default_rng(1000 + seed)
    users, tables = random_level(oracle, rng)
    batches = []
    for seq in (23, 25, 27, 2**63 - 1, 0):
        keys = [users[int(i)] for i in rng.integers(0, len(users), 50)]
        keys += [oracle._decode_inner(t[1])[0] for t in tables[:8]]  # max user keys: the seq-dependent case
        keys += [b"", b"a", b"zzz", users[0] + b"\x00", users[-1] + b"\xff"]
        batches.append((keys, seq))
    got = index_candidates(g, tables, batches)
    dropped_somewhere = False
    for (keys, seq), per_key in zip(batches, got):
        fresh = fresh_candidates(f, tables, keys, seq)
        for i, k in enumerate(keys):
            want = oracle.level_candidates(tables, k, seq)
            assert per_key[i] == want, (seq, i, k)
            assert fresh[i] == want, (seq, i, k)
            dropped_somewhere |= want != oracle.level_candidates(tables, k, 2**63 - 1)
    assert dropped_somewhere  # the batches do differ by seq


def test_equality_op_cases_explicit(mirror, oracle):
    """max seq below, equal (op 0 and op 1) and above the lookup's seq at a
    table's own max user key."""
    f, g = mirror
    tables = [(inner(b"a", 9, 0), inner(b"m", 24, 0)), (inner(b"b", 9, 0), inner(b"m", 25, 0)),
              (inner(b"c", 9, 0), inner(b"m", 25, 1)), (inner(b"d", 9, 0), inner(b"m", 26, 0)),
              (inner(b"e", 9, 0), inner(b"z", 3, 0))]
    got = index_candidates(g, tables, [([b"m", b"l", b"n"], s) for s in (24, 25, 26)])
    assert got[0][0] == [4, 0] and got[1][0] == [4, 1, 0] and got[2][0] == [4, 3, 2, 1, 0]
    for per_key, seq in zip(got, (24, 25, 26)):
        assert per_key[1] == [4, 3, 2, 1, 0] and per_key[2] == [4]
        for k, lst in zip([b"m", b"l", b"n"], per_key):
            assert lst == oracle.level_candidates(tables, k, seq)


def overlapping_tables(n):
    return [(inner(b"u%05d" % t, 9, 1), inner(b"v%05d" % t, 9, 1)) for t in range(n)]


def test_over_budget_reports_too_large_and_nothing_else():
    """64 mutually overlapping tables need about 64^2 list entries: a tiny
    budget refuses the index (ADL_ERR_TOO_LARGE), the default one builds it.
    create and stats need no GPU."""
    import adlbloom

    tables = overlapping_tables(64)
    with pytest.raises(adlbloom.AdlBloomError) as e:
        adlbloom.LevelIndex(tables, max_index_bytes=4096)
    assert e.value.status == adlbloom.ADL_ERR_TOO_LARGE
    lv = adlbloom.LevelIndex(tables)
    regions, entries, nbytes, longest = lv.stats()
    assert regions == 2 * 128 + 1 and longest == 64
    # sum over regions of the active tables: 2 * (0 + 1 + ... + 63) in the gaps, 64 more per point region
    assert entries == 2 * sum(range(64)) + 64 + sum(range(1, 65)) * 2
    assert 4 * entries < nbytes <= 256 << 20
    lv.close()


def test_over_budget_in_the_mirror(mirror):
    f, g = mirror
    tables = overlapping_tables(64)
    mins, ml = _arr([t[0] for t in tables])
    maxs, xl = _arr([t[1] for t in tables])
    ks, kl = _arr([b"u00001"])
    kb = np.array([0, 1], dtype=np.uint32)
    seqs = np.array([5], dtype=np.int64)
    begin, table = np.zeros(2, np.uint32), np.zeros(65, np.uint32)
    args = (ks, kl.ctypes.data, kb.ctypes.data, 1, seqs.ctypes.data, begin.ctypes.data, table.ctypes.data, 65)
    assert g(mins, ml.ctypes.data, maxs, xl.ctypes.data, 64, 4096, *args) == -2
    assert g(mins, ml.ctypes.data, maxs, xl.ctypes.data, 64, 0, *args) == 2  # tables 0 and 1 cover u00001
