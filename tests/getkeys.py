"""Single-key Get requests of the resident probe server's fan form (one key,
n tables, adlsm-tree_amd/csrc/probe_server.hip), shared by
tests/test_revision_get_cpu.py (which proves, without a GPU, that the table
holds what it claims) and tests/test_gpu_revision_get.py (which sends every
call through FilterCache.probe_key).

Built on tests/serverkeys.py's geometry (its ten tables of k = 1 .. 30 over one
member set, its multi-filter table, its 2^13 -+ 8-bit tables, its never-cached
oid) plus, here:
  M56, M128, M8192   one-filter blocks (bits_per_key 9) over 0, 1 and 113 keys:
                     m = 56 (the minimum), 128 and 2^13 bits
  REMOVED            a block that is put and then removed (answers 1, counted)
  SOLO0 .. SOLO0+23  24 one-key blocks (bits_per_key 10) over 24 distinct keys,
                     key j a member of block j alone (the oracle says so, the
                     CPU test asserts it): "exactly table j answers 1" reaches
                     every answer bit of the three tagged words

Expected answers come from one oracle.probe call per (table, filter) over the
pool of every key a call uses.  Everything is deterministic from fixed seeds;
nothing here imports the GPU side.
"""
import functools
from typing import NamedTuple

import numpy as np

import oracle as O
import serverkeys as SK

MAX_TABLES = 24     # ADL_BLOOM_GET_MAX_TABLES
MAX_KEY_BYTES = 96  # ADL_BLOOM_GET_MAX_KEY_BYTES
COUNTS = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25)
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 40, 41, 95, 96, 97)
# serverkeys' tables by k: 1, 5, 6, 7, 12, 13, 30 -- around the groups of kReads = 6 bit reads
K_TABLES = tuple(SK.KS.index(k) for k in (1, 5, 6, 7, 12, 13, 30))

M56, M128, M8192 = SK.T_UNCACHED + 1, SK.T_UNCACHED + 2, SK.T_UNCACHED + 3
REMOVED = M8192 + 1
SOLO0 = REMOVED + 1
NTABLES = SOLO0 + MAX_TABLES


class Get(NamedTuple):
    key: bytes
    tables: tuple    # table index per candidate
    filter: int
    path: str        # "server" | "launched"


class Case(NamedTuple):
    name: str
    calls: tuple


def eligible(n, nbytes):
    """adl_srv::eligible_fan."""
    return 1 <= n <= MAX_TABLES and nbytes <= MAX_KEY_BYTES


def get(key, tables, filter=0):
    tables = tuple(int(t) for t in tables)
    return Get(bytes(key), tables, filter, "server" if eligible(len(tables), len(key)) else "launched")


class GetGeometry:
    def __init__(self):
        G = self.G = SK.load()
        multi = G.tables[SK.T_MULTI].members
        self.tables = list(G.tables)
        for name, idx in ((b"get-m56", multi[0]), (b"get-m128", multi[1]), (b"get-m8192", multi[2])):
            self.tables.append(SK._table(name, 9, G.flat, [list(idx)]))
        self.tables.append(SK._table(b"get-removed", 10, G.flat, [list(range(8, 400))]))
        self._solo()
        assert len(self.tables) == NTABLES
        self.oids = [t.oid for t in self.tables]
        self.never_resident = (SK.T_UNCACHED, REMOVED)
        self.cases = _cases(self)
        pool = sorted({c.key for case in self.cases for c in case.calls})
        self.pool = {k: i for i, k in enumerate(pool)}
        self.truth = {}
        for t, tab in enumerate(self.tables):
            for f, bm in enumerate(tab.bitmaps):
                self.truth[t, f] = O.probe(pool, bm, bits_per_key=tab.bpk)
        self._expected = {}

    def _solo(self):
        """24 one-key blocks; key j answers 1 in block j and 0 in the other 23,
        and `nobody` answers 0 in all of them (redrawn until the oracle agrees)."""
        rng = np.random.default_rng(0x5010)
        for _ in range(50):
            keys = [rng.integers(0, 256, 5 + 3 * j, dtype=np.uint8).tobytes() for j in range(MAX_TABLES)]
            nobody = rng.integers(0, 256, 33, dtype=np.uint8).tobytes()
            bms = [O.keys2block([k], bits_per_key=10) for k in keys]
            ans = np.array([O.probe(keys + [nobody], bm, bits_per_key=10) for bm in bms])
            if np.array_equal(ans[:, :MAX_TABLES], np.eye(MAX_TABLES, dtype=ans.dtype)) and not ans[:, MAX_TABLES].any():
                break
        else:
            raise AssertionError("no 24 keys that are members of their own block alone")
        self.solo_keys, self.nobody = keys, nobody
        for j, (k, bm) in enumerate(zip(keys, bms)):
            self.tables.append(SK.Table(b"get-solo-%d" % j, 10, O.filter_block_final([bm.tobytes()], 10), (bm,), ((),)))

    def resident(self, t):
        return t not in self.never_resident

    def expected(self, c):
        """The oracle's answers of a call of self.cases (read-only; shared by every caller)."""
        if c not in self._expected:
            out = np.empty(len(c.tables), np.uint8)
            for i, t in enumerate(c.tables):
                if not self.resident(t):
                    out[i] = 1                                   # not cached: may be present
                elif c.filter >= len(self.tables[t].bitmaps):
                    out[i] = 0                                   # no such filter in the block
                else:
                    out[i] = self.truth[t, c.filter][self.pool[c.key]]
            out.setflags(write=False)
            self._expected[c] = out
        return self._expected[c]

    def uncached(self, c):
        return sum(not self.resident(t) for t in c.tables)


def _cases(g):
    G = g.G
    cases = []
    # count-n: n candidates over the ten k; a member of all of them, and a key none of them holds
    for n in COUNTS:
        tabs = [(3 * i + n) % SK.NT for i in range(n)]
        cases.append(Case("count-%d" % n, (get(G.member(16, n), tabs), get(G.universal[1], tabs),
                                           get(G.member(41, n + 1), tabs[::-1]))))
    # bit-j: 24 candidates, exactly table j answers 1; all of them; none
    solo = list(range(SOLO0, SOLO0 + MAX_TABLES))
    for j in range(MAX_TABLES):
        cases.append(Case("bit-%d" % j, (get(g.solo_keys[j], solo),)))
    cases.append(Case("bit-none", (get(g.nobody, solo),)))
    all24 = [(7 * i) % SK.NT for i in range(MAX_TABLES)]
    cases.append(Case("bit-all", (get(G.member(33, 1), all24),)))
    # len-L: every member kind (random, every byte >= 0x80, the sign-extended tail) and two non-members,
    # against tables that hold the members and tables that do not
    for L in LENGTHS:
        calls = []
        for kind in range(4):
            calls.append(get(G.member(L, kind), [(L + kind) % SK.NT, SK.T_LO, (L + kind + 5) % SK.NT, M8192, SK.T_HI]))
        if L:
            for t in ((L + 4) % SK.NT, (L + 7) % SK.NT):
                calls.append(get(G.non[t][L], [(t + 1) % SK.NT, t, SK.T_LO, t, M128]))
        cases.append(Case("len-%d" % L, tuple(calls)))
    # mixed: every k around kReads, m = 56, 128, 2^13 and 2^13 -+ 8, an uncached and a removed table
    mixed = list(K_TABLES) + [M56, M128, M8192, SK.T_LO, SK.T_HI, SK.T_UNCACHED, REMOVED, SK.T_MULTI]
    multi = G.tables[SK.T_MULTI].members
    keys = [G.member(40, 0), G.universal[2], G.flat[multi[2][0]], G.flat[multi[1][0]],
            G.flat[G.tables[SK.T_LO].members[0][5]], G.flat[G.tables[SK.T_HI].members[0][7]], b""]
    cases.append(Case("mixed", tuple(get(k, mixed) for k in keys) + tuple(get(k, mixed[::-1]) for k in keys[:3])))
    # no-such-filter: filter 1 and 2 exist in the multi-filter block alone, filter 3 nowhere
    lack = [SK.T_MULTI, 3, M128, SK.T_UNCACHED, 5, SK.T_MULTI]
    cases.append(Case("no-such-filter", (get(G.flat[multi[1][0]], lack, filter=1), get(G.flat[multi[2][3]], lack, filter=2),
                                         get(G.universal[0], lack, filter=2), get(G.flat[multi[2][3]], lack, filter=3))))
    return cases


@functools.lru_cache(maxsize=None)
def load():
    return GetGeometry()


def by_name(g):
    return {case.name: case for case in g.cases}
