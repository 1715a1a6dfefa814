"""Request geometries of the resident probe server (adlsm-tree_amd/csrc/
probe_server.hip), shared by tests/test_probe_server_cases_cpu.py (which
proves, without a GPU, that the table holds what it claims) and
tests/test_gpu_probe_server_geometry.py (which sends every call to the server).

Everything is deterministic from fixed seeds; nothing here imports the GPU side.

Tables (load().tables, indices into load().oids):
  0..9      one one-filter block per bits_per_key in BPKS (k = KS), all over ONE
            member set: four keys of every length 0..320 (two of random bytes,
            one with every byte >= 0x80, one whose last len & 3 bytes are
            >= 0x80 and the rest < 0x80: the sign-extended tail)
  T_MULTI   bits_per_key 9, three filters over 0, 1 and 113 member keys:
            m = 56 (the minimum), 128 and 8192 = 2^13 bits; filter index 3
            does not exist
  T_LO/T_HI bits_per_key 1 over 1016 / 1018 member keys: m = 2^13 - 8 / + 8
  T_UNCACHED an oid that is never put (answers 1: "may be present")

Non-members: for every table 0..9 and every length 1..320 one key the oracle
answers 0, redrawn from a fixed seed until it does (load().redraws counts).
Length 0 has one key only, the empty one, and the member set holds it: its
expected 0 can only come from a table that does not hold it (T_MULTI's
filters, T_LO, T_HI), and the `len-0` case asks those.

Expected answers come from one oracle.probe call per (table, filter) over the
pool of every key a case uses, not from a call per request.
"""
import functools
from typing import NamedTuple

import numpy as np

import oracle as O

MAXLEN = 320   # adl_srv::kMaxKeyBytes: key bytes per served request
MAXQ = 8       # adl_srv::kMaxQ: queries per served request
INLINE = 40    # kInlineKeyBytes: a one-query request of slots 0-3 sits in its bell line
BPKS = (1, 3, 8, 9, 11, 16, 18, 19, 43, 44)
KS = (1, 2, 5, 6, 7, 11, 12, 13, 29, 30)  # int(bpk * 0.69) clamped to 1..30; kReads = 6 per group
NT = len(BPKS)
T_MULTI, T_LO, T_HI, T_UNCACHED = NT, NT + 1, NT + 2, NT + 3
MULTI_COUNTS = (0, 1, 113)
EDGE_COUNTS = {T_LO: 1016, T_HI: 1018}
KINDS = ("random-a", "random-b", "high", "tail")


class Call(NamedTuple):
    keys: tuple      # bytes per query
    tables: tuple    # table index per query
    filter: int      # filter index of the call
    form: str        # "offsets" | "stride" (every key of one length) | "base" (offsets[0] = base > 0)
    base: int        # "base": bytes in front of the first key
    path: str        # "server" | "launched"

    @property
    def nbytes(self):
        return sum(len(k) for k in self.keys)


class Case(NamedTuple):
    name: str
    calls: tuple


class Table(NamedTuple):
    oid: bytes
    bpk: int
    block: bytes        # None: never put
    bitmaps: tuple      # one uint8 array per filter
    members: tuple      # per filter: indices into load().flat


def _members():
    rng = np.random.default_rng(0x5E12E1)
    out = []
    for L in range(MAXLEN + 1):
        a = rng.integers(0, 256, L, dtype=np.uint8)
        b = rng.integers(0, 256, L, dtype=np.uint8)
        hi = rng.integers(0x80, 256, L, dtype=np.uint8)
        t = rng.integers(0, 0x80, L, dtype=np.uint8)
        r = L & 3
        if r:
            t[L - r:] = rng.integers(0x80, 256, r, dtype=np.uint8)
        out.append(tuple(x.tobytes() for x in (a, b, hi, t)))
    return out


def _table(oid, bpk, flat, member_lists):
    bms = tuple(O.keys2block([flat[i] for i in idx], bits_per_key=bpk) for idx in member_lists)
    return Table(oid, bpk, O.filter_block_final([bm.tobytes() for bm in bms], bpk), bms,
                 tuple(tuple(idx) for idx in member_lists))


class Geometry:
    def __init__(self):
        self.members = _members()                               # [L][kind]
        self.flat = [k for four in self.members for k in four]  # index 4 L + kind
        n = len(self.flat)
        every = list(range(n))
        self.tables = [_table(b"geo-bpk%d" % b, b, self.flat, [every]) for b in BPKS]
        rng = np.random.default_rng(0x7AB1E5)
        # (none of the three smaller blocks holds the empty key, flat[0..3])
        multi = [[], [4 * 40 + 1], sorted(int(i) for i in 4 + rng.choice(n - 4, MULTI_COUNTS[2], replace=False))]
        self.tables.append(_table(b"geo-multi", 9, self.flat, multi))
        for t in (T_LO, T_HI):
            idx = sorted(int(i) for i in 4 + rng.choice(n - 4, EDGE_COUNTS[t], replace=False))
            self.tables.append(_table(b"geo-edge-%d" % EDGE_COUNTS[t], 1, self.flat, [idx]))
        self.tables.append(Table(b"geo-not-cached", 0, None, (), ()))
        self.oids = [t.oid for t in self.tables]
        self._nonmembers()
        self._universal()
        self.cases = _cases(self)
        self._truth()

    # ---- keys
    def member(self, L, kind):
        return self.members[L][kind % 4]

    def _nonmembers(self):
        rng = np.random.default_rng(0xA85E17)
        self.non = [[None] * (MAXLEN + 1) for _ in range(NT)]   # [table][L], L >= 1
        self.redraws = np.zeros((NT, MAXLEN + 1), np.int64)
        for t in range(NT):
            todo = list(range(1, MAXLEN + 1))
            for _ in range(200):
                if not todo:
                    break
                cand = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in todo]
                ans = O.probe(cand, self.tables[t].bitmaps[0], bits_per_key=BPKS[t])
                again = []
                for L, c, a in zip(todo, cand, ans):
                    if a == 0:
                        self.non[t][L] = c
                    else:
                        self.redraws[t][L] += 1
                        again.append(L)
                todo = again
            assert not todo, ("no non-member found", t, todo)

    def _universal(self):
        """Four keys the oracle answers 0 in every one of the ten tables (k-sweep)."""
        rng = np.random.default_rng(0x0A11)
        self.universal = []
        for L in (7, 16, 33, 64):
            for _ in range(200):
                c = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
                if not any(int(O.probe([c], self.tables[t].bitmaps[0], bits_per_key=BPKS[t])[0]) for t in range(NT)):
                    break
            else:
                raise AssertionError("no key absent from all ten tables")
            self.universal.append(c)

    # ---- expected answers: one oracle call per (table, filter) over the pool
    def _truth(self):
        pool = sorted({k for case in self.cases for c in case.calls for k in c.keys})
        self.pool = {k: i for i, k in enumerate(pool)}
        self.truth, self._expected = {}, {}
        for t, tab in enumerate(self.tables):
            for f, bm in enumerate(tab.bitmaps):
                self.truth[t, f] = O.probe(pool, bm, bits_per_key=tab.bpk)

    def expected(self, call):
        """The oracle's answers of a call of self.cases (read-only; shared by every caller)."""
        if call not in self._expected:
            self._expected[call] = self._expect(call)
        return self._expected[call]

    def _expect(self, call):
        out = np.empty(len(call.keys), np.uint8)
        for i, (k, t) in enumerate(zip(call.keys, call.tables)):
            if t == T_UNCACHED:
                out[i] = 1                                   # not cached: may be present
            elif call.filter >= len(self.tables[t].bitmaps):
                out[i] = 0                                   # no such filter in the block
            else:
                out[i] = self.truth[t, call.filter][self.pool[k]]
        out.setflags(write=False)
        return out

    def uncached(self, call):
        return sum(t == T_UNCACHED for t in call.tables)


def eligible(n, nbytes):
    """adl_srv::eligible."""
    return 1 <= n <= MAXQ and nbytes <= MAXLEN


def call(keys, tables, filter=0, form="offsets", base=0):
    keys, tables = tuple(keys), tuple(tables)
    assert len(keys) == len(tables)
    if form == "stride":
        assert len({len(k) for k in keys}) == 1 and len(keys[0]) > 0
    return Call(keys, tables, filter, form, base,
                "server" if eligible(len(keys), sum(len(k) for k in keys)) else "launched")


def materialise(c):
    """(keys array, offsets or None) as FilterCache.probe takes them."""
    if c.form == "stride":
        return np.frombuffer(b"".join(c.keys), np.uint8).reshape(len(c.keys), len(c.keys[0])).copy(), None
    lead = bytes((0xC3 ^ i) & 0xFF for i in range(c.base)) if c.form == "base" else b""
    data = np.frombuffer(lead + b"".join(c.keys) + b"\0", np.uint8).copy()
    offs = (len(lead) + np.concatenate([[0], np.cumsum([len(k) for k in c.keys])])).astype(np.uint64)
    return data, offs


def pack_lengths(n, r, total):
    """n key lengths adding up to `total`, the first of r bytes (so the second
    key starts at offset r of the slot's key area), an empty key in the middle
    and one at the end where n allows both (n = 3: the middle for even r, the
    end for odd r; n = 2: neither).  No key is longer than 320 bytes: where
    one key takes all the rest (n <= 4) and r leaves it 321, the first key gets
    r + 1."""
    if n <= 4 and total - r > MAXLEN:
        r += 1
    if n == 2:
        return [r, total - r]
    if n == 3:
        return [r, 0, total - r] if r % 2 == 0 else [r, total - r, 0]
    m = n - 3  # keys besides the first and the two empty ones
    rest = total - r
    piece = [rest // m + (2 * j + 1) * (-1) ** j for j in range(m - 1)]
    piece.append(rest - sum(piece))
    assert all(0 < p <= MAXLEN for p in piece)
    lens = [r] + piece
    lens.insert(n // 2, 0)
    lens.append(0)
    assert len(lens) == n and sum(lens) == total
    return lens


def _mixed(G, lens, salt):
    """Keys of the given lengths, members and non-members in turn over several
    tables: the first non-empty key a member, the last a non-member (a request
    with one non-empty key: a non-member beside the empty member)."""
    nonempty = [i for i, L in enumerate(lens) if L]
    keys, tables = [], []
    for i, L in enumerate(lens):
        t = (salt + 3 * i) % NT
        is_member = L == 0 or (nonempty.index(i) % 2 == 0 and i != nonempty[-1])
        keys.append(G.member(L, i + salt) if is_member else G.non[t][L])
        tables.append(t)
    return keys, tables


def _cases(G):
    cases = []
    # len-L: one query, every member kind and two non-members, tables in turn
    for L in range(MAXLEN + 1):
        calls = [call([G.member(L, kind)], [(L + kind) % NT], form="stride" if L and kind % 2 else "offsets")
                 for kind in range(4)]
        if L:
            calls += [call([G.non[t][L]], [t]) for t in ((L + 4) % NT, (L + 7) % NT)]
        else:
            calls += [call([b""], [T_LO]), call([b""], [T_HI]), call([b""], [T_MULTI]),
                      call([b""], [T_MULTI], filter=1), call([b""], [T_MULTI], filter=2)]
        cases.append(Case("len-%d" % L, tuple(calls)))
    # pack-n-r: n keys of exactly 320 bytes (served) and of 321 (launched)
    for n in range(2, MAXQ + 1):
        for r in range(8):
            calls = [call(*_mixed(G, pack_lengths(n, r, total), n + r)) for total in (MAXLEN, MAXLEN + 1)]
            cases.append(Case("pack-%d-%d" % (n, r), tuple(calls)))
    # stride-s: a fixed stride instead of an offsets array
    for s in (1, INLINE, INLINE + 1, MAXLEN):
        cases.append(Case("stride-%d" % s, (call([G.member(s, 1)], [s % NT], form="stride"),
                                            call([G.non[(s + 5) % NT][s]], [(s + 5) % NT], form="stride"))))
    for s in (INLINE, INLINE + 1):  # 8 x 40 = 320 bytes: served; 8 x 41 = 328: launched
        keys, tables = _mixed(G, [s] * MAXQ, s)
        cases.append(Case("stride-%dx8" % s, (call(keys, tables, form="stride"),)))
    # offs-base: offsets that do not start at 0 (also past the 320 bytes a request may hold)
    keys, tables = _mixed(G, [5, 0, 41, 40, 13], 2)
    cases.append(Case("offs-base", (call(keys, tables, form="base", base=37),
                                    call([G.member(INLINE, 2)], [4], form="base", base=3),
                                    call([G.non[6][INLINE + 1]], [6], form="base", base=1),
                                    call(*_mixed(G, [100, 0, 99, 1], 5), form="base", base=301))))
    # n9: one query more than a request holds
    keys, tables = _mixed(G, [16] * (MAXQ + 1), 1)
    cases.append(Case("n9", (call(keys, tables), call(keys, tables, form="stride"))))
    # alt-40-41: the inline and the slot form in turn on one slot (the bell's bit 31 flips)
    cases.append(Case("alt-40-41", tuple(call([G.member(INLINE + i % 2, i // 2)], [i % NT]) for i in range(16))))
    cases.append(Case("alt-40-41-absent",
                      tuple(call([G.non[(3 * i) % NT][INLINE + i % 2]], [(3 * i) % NT]) for i in range(16))))
    # k-sweep: the same 8 keys against every table, then the ten k mixed in a request
    same = [G.member(9, 0), G.universal[0], G.member(24, 2), G.universal[1], G.member(40, 3), G.universal[2],
            G.member(41, 1), G.universal[3]]
    calls = [call(same, [t] * MAXQ) for t in range(NT)]
    calls += [call(same, list(range(0, 8))), call(same, list(range(NT - 1, 1, -1)))]
    cases.append(Case("k-sweep", tuple(calls)))
    # the divisor classes: m = 56, 128 and 2^13 (T_MULTI's filters), 2^13 -+ 8 (T_LO, T_HI)
    multi = G.tables[T_MULTI].members
    for f in range(3):
        ins = [G.flat[i] for i in multi[f][:3]]
        outs = [G.flat[i] for i in sorted(set(multi[2]) - set(multi[f]))[:2]] + [G.non[3][77], G.non[3][200]]
        keys = sorted(ins + outs, key=len)  # the shortest first: as many as fit in a request
        while sum(len(k) for k in keys) > MAXLEN - 20:
            keys.pop()
        # (filter 0 holds no key and answers 0 throughout: with filter=0 a member asked of table 3 gives the
        # request its 1; with filter 1 or 2 that table has no such filter)
        both = call(keys + [G.member(20, f)], [T_MULTI] * len(keys) + [3], filter=f)
        cases.append(Case("multi-f%d" % f, (both,) + tuple(call([k], [T_MULTI], filter=f) for k in keys)))
    for t in (T_LO, T_HI):
        ins = [G.flat[i] for i in G.tables[t].members[0][5::211]]
        outs = [G.non[0][L] for L in (3, 40, 41, 150)]
        cases.append(Case("edge-%d" % EDGE_COUNTS[t], tuple(call([k], [t]) for k in ins + outs)))
    # uncached, no-such-filter: as tests/test_gpu_readpath.py expects them
    keys, tables = _mixed(G, [12, 40, 0, 41, 64], 7)
    tables[1] = tables[3] = T_UNCACHED
    cases.append(Case("uncached", (call(keys, tables), call([G.non[2][40]], [T_UNCACHED]),
                                   call([G.member(200, 0)], [T_UNCACHED]))))
    tables[0] = T_MULTI
    cases.append(Case("no-such-filter", (call(keys, tables, filter=1), call([G.member(40, 0)], [5], filter=1),
                                         call([G.member(41, 0)], [5], filter=1),
                                         call([G.flat[multi[2][0]]], [T_MULTI], filter=3))))
    return cases


@functools.lru_cache(maxsize=None)
def load():
    return Geometry()
