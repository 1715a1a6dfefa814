"""Revisions the revision tests share (tests/test_revision_cpu.py,
tests/test_gpu_revision.py): lists of tests/test_gpu_level_index.py's level
shapes in Revision::Get's visiting order, a lookup pool aimed at the boundaries
of all of them, and the expected candidate lists -- oracle.level_candidates per
level, concatenated level 0 first, shifted to global table ids.

For the scale tests (tests/test_revision_scale_cpu.py,
tests/test_gpu_revision_scale.py): a disjoint level of T tables whose candidate
lists have a closed form, revisions of more than 8 192 and more than 65 536
tables built on it, and references that work on CPU and on device tensors
alike -- the hit lists gathered from a truth table, the grouping by table, and
comparers that bring back only counts and first indices."""
import numpy as np

from levelkeys import inner, max_tail
from test_gpu_level_index import _level, _pool

# None: a missing level (NULL); "empty": a level of no tables
REVISIONS = {
    "one": ("t16",),
    "two": ("t3", "t16"),
    "five": ("t3", "empty", None, "t16", "t300"),
    "eight": ("t1", "t3", "t16", "t3", "t257", "t16", "t1", "t3"),  # ADL_BLOOM_MAX_LEVELS, none empty
    "twice300": ("t300", "t300"),  # one key with 600 candidates: more than two rounds of a workgroup
    "wide": ("t257", "t16"),       # 514 boundaries (searched in global memory) beside 50 (staged in LDS)
}
SEQS = (24, 25, 26)  # the tables' max seqs are 24, 25 (op 0 and op 1) and 26

_tables = {}
_lists = {}
_pools = {}


def tables(name):
    """[(min_inner, max_inner)] of a level shape; [] for "empty" and for None."""
    if name in (None, "empty"):
        return []
    if name not in _tables:
        # "d<T>": the disjoint level of T tables (below); every other name is a shape of test_gpu_level_index
        _tables[name] = disjoint_level(int(name[1:])) if name[0] == "d" and name[1:].isdigit() else _level(name)
    return _tables[name]


def table_base(names):
    return np.concatenate([[0], np.cumsum([len(tables(n)) for n in names])]).astype(np.uint32)


def pool(names, stride=None, per_level=70):
    """Distinct lookup keys: up to per_level of each distinct level's pool
    (test_gpu_level_index._pool: every boundary feature), and the keys every
    pool has.  stride: None for var-len keys, else every key of that size."""
    key = (names, stride, per_level)
    if key not in _pools:
        keys = set()
        for n in sorted({n for n in names if n not in (None, "empty")}):
            p = _pool(tables(n), stride)
            rng = np.random.default_rng(len(p))
            keys |= set(p if len(p) <= per_level else [p[int(i)] for i in rng.choice(len(p), per_level, replace=False)])
        fixed = [b"", b"ab", b"ab\0", b"\x65", b"\xff\xff\xff", bytes(300)]
        keys |= {(k + bytes(stride))[:stride] for k in fixed} if stride else set(fixed)
        _pools[key] = sorted(keys)
    return _pools[key]


def level_list(oracle, name, key, seq):
    k = (name, key, seq)
    if k not in _lists:
        _lists[k] = oracle.level_candidates(tables(name), key, seq)
    return _lists[k]


def revision_lists(oracle, names, keys, seq):
    """Per key: the global ids of its candidates, level 0 first."""
    base = table_base(names)
    out = []
    for k in keys:
        row = []
        for l, n in enumerate(names):
            if tables(n):
                row += [int(base[l]) + t for t in level_list(oracle, n, k, seq)]
        out.append(row)
    return out


def csr(lists):
    begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    flat = np.array([t for x in lists for t in x], np.uint32)
    return begin, flat


def gather_lists(lists, sel):
    """csr([lists[i] for i in sel]) for a long `sel` (no Python loop over it)."""
    sel = np.asarray(sel, np.int64)
    lens = np.array([len(x) for x in lists], np.int64)
    start = np.cumsum(lens) - lens
    flat = np.array([t for x in lists for t in x] + [0], np.uint32)
    cnt = lens[sel]
    begin = np.concatenate([[0], np.cumsum(cnt)])
    owner = np.repeat(np.arange(len(sel)), cnt)
    at = start[sel][owner] + (np.arange(int(begin[-1])) - begin[owner])
    return begin.astype(np.uint32), flat[at]


# ------------------------------------------------------------------ the disjoint level and its revisions
def disjoint_level(T):
    """T tables with disjoint ranges: table i holds the user keys "d%06d" % i + "a" to "d%06d" % i + "z"."""
    return [(inner(b"d%06d" % i + b"a", 9, 0), inner(b"d%06d" % i + b"z", *max_tail(i))) for i in range(T)]


DISJOINT_KINDS = (b"m", b"n", b"zz")


def disjoint_key(i, kind):
    """b"m", b"n": inside table i's range; b"zz": behind its max user key and before the next table's min."""
    assert kind in DISJOINT_KINDS
    return b"d%06d" % i + kind


def disjoint_list(i, kind):
    """The closed form of oracle.level_candidates(disjoint_level(T), disjoint_key(i, kind), seq) for i < T:
    the users differ from both boundaries, so no seq matters (tests/test_revision_scale_cpu.py holds it
    against the oracle)."""
    return [] if kind == b"zz" else [i]


def disjoint_list_of_other(key):
    """The closed form for a key that does not start with "d": every boundary of the level does, so the key
    lies before the first min or behind the last max whatever T and seq are (held against the oracle in
    tests/test_revision_scale_cpu.py)."""
    assert not key.startswith(b"d")
    return []


# the disjoint level first, so that t16's global ids are the highest
SCALE_REVISIONS = {
    "d8176": ("d8176", "t16"),    # 8 192 tables: the most whose group arrays ride with the counts
    "d8177": ("d8177", "t16"),    # 8 193: the fewest whose group arrays come as pieces of their own
    "d9000": ("d9000", "t16"),
    "d65600": ("d65600", "t16"),  # ids of 17 bits: three sort passes
}
D_LOWEST, D_HIGHEST = b"d", b"d" + b"\xff" * 12
_d16 = {}


def t16_list_of_d(oracle, seq):
    """t16's candidates of any key that starts with "d": no t16 boundary starts with it, so the lowest and the
    highest such key lie in one region and have the oracle's same list."""
    if seq not in _d16:
        for mn, mx in tables("t16"):
            for k in (mn, mx):
                assert not (k[:-9] if len(k) >= 9 else k).startswith(b"d")
        lo, hi = level_list(oracle, "t16", D_LOWEST, seq), level_list(oracle, "t16", D_HIGHEST, seq)
        assert lo == hi
        _d16[seq] = lo
    return _d16[seq]


def scale_list(oracle, T, i, kind, seq):
    """The global ids of disjoint_key(i, kind) in the revision (dT, t16)."""
    return disjoint_list(i, kind) + [T + t for t in t16_list_of_d(oracle, seq)]


# ------------------------------------------------------------------ filters over a small pool of keys
def filters_of_a_pool(oracle, rng, npool, F, bpks, stride, empty=None):
    """npool distinct keys (var-len of 1 to 39 bytes, or all of `stride` bytes) and F filters, each built by the
    oracle from a random subset of them with bits_per_key bpks[f % len(bpks)]; filter `empty` has no bytes.
    -> (pool, bitmaps uint8 with 16 spare bytes, bitmap_off uint64[F + 1], bits_per_key int[F])"""
    pool = sorted({rng.integers(0, 256, stride or int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
                   for _ in range(npool * 3)})[:npool]
    assert len(pool) == npool
    bpk = np.array([bpks[f % len(bpks)] for f in range(F)])
    bms = []
    for f in range(F):
        members = [pool[int(i)] for i in np.flatnonzero(rng.random(npool) < 0.4)] or [pool[f % npool]]
        bms.append(b"" if f == empty else oracle.keys2block(members, bits_per_key=int(bpk[f])).tobytes())
    off = np.concatenate([[0], np.cumsum([len(b) for b in bms])]).astype(np.uint64)
    return pool, np.frombuffer(b"".join(bms) + bytes(16), np.uint8), off, bpk


# ------------------------------------------------------------------ references on tensors (CPU or device)
def truth_table(oracle, pool, bitmaps, bitmap_off, bits_per_key):
    """uint8[len(pool), F + 1]: oracle.probe_multi of every pool key against every filter.  An empty filter
    answers 0 (include/adl_bloom.h), and so does the last column, which stands for every id >= F.
    bits_per_key: one value, or one per filter."""
    off = np.asarray(bitmap_off, np.uint64)
    F = len(off) - 1
    bpk = np.broadcast_to(np.asarray(bits_per_key), (F,))
    truth = np.zeros((len(pool), F + 1), np.uint8)
    for b in np.unique(bpk):
        f = np.flatnonzero((bpk == b) & (np.diff(off.astype(np.int64)) > 0))
        if len(f):
            keys = [k for k in pool for _ in range(len(f))]
            truth[:, f] = oracle.probe_multi(keys, np.tile(f, len(pool)), bitmaps, off,
                                             bits_per_key=int(b)).reshape(len(pool), len(f))
    return truth


def expected_hits(torch, truth, sel, pair_begin, pair_filter):
    """The hit lists of keys pool[sel] with the pairs (pair_begin int64[K+1], pair_filter int64[P]): the answers
    gathered from `truth` (a uint8 tensor of truth_table) by (sel[owner], pair_filter), the pairs answered 1
    kept in pair order.  -> (hit_begin int64[K+1], hit_filter int64[H], answers uint8[P])"""
    K, P = sel.numel(), pair_filter.numel()
    dev = sel.device
    owner = torch.repeat_interleave(torch.arange(K, device=dev), pair_begin[1:] - pair_begin[:-1], output_size=P)
    ans = truth[sel[owner], pair_filter.clamp(max=truth.shape[1] - 1)]
    per_key = torch.zeros(K, dtype=torch.int64, device=dev).index_add_(0, owner, ans.to(torch.int64))
    hit_begin = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    hit_begin[1:] = torch.cumsum(per_key, 0)
    return hit_begin, pair_filter[ans.bool()], ans


def torch_plan(torch, hit_begin, hit_table):
    """test_read_plan_cpu.expected_plan on tensors (int64, CPU or device): a stable sort of the ids, the owners
    from repeat_interleave, the groups from unique_consecutive.  -> (group_table, group_begin, entry_key)"""
    K, H = hit_begin.numel() - 1, hit_table.numel()
    dev = hit_begin.device
    owner = torch.repeat_interleave(torch.arange(K, device=dev), hit_begin[1:] - hit_begin[:-1], output_size=H)
    ids, order = torch.sort(hit_table, stable=True)
    tabs, counts = torch.unique_consecutive(ids, return_counts=True)
    begin = torch.zeros(tabs.numel() + 1, dtype=torch.int64, device=dev)
    begin[1:] = torch.cumsum(counts, 0)
    return tabs, begin, owner[order]


def unsigned(torch, t):
    """An int32 tensor that holds the library's u32, widened."""
    return t.to(torch.int64) & 0xFFFFFFFF if t.dtype == torch.int32 else t.to(torch.int64)


def compare_where_they_live(torch, **pairs):
    """name=(got, want), tensors on one device (int32 read as u32, or int64), the first len(want) entries of
    got compared.  Only counts and first indices come back: {name_bad, name_first}; a `got` that is too short
    counts as len(want) bad entries, the first at its own length."""
    out = {}
    for name, (got, want) in pairs.items():
        n = want.numel()
        if got.numel() < n:
            out[name + "_bad"], out[name + "_first"] = n, got.numel()
            continue
        bad = unsigned(torch, got[:n]) != unsigned(torch, want)
        count = int(bad.sum().item())
        out[name + "_bad"] = count
        out[name + "_first"] = int(bad.to(torch.uint8).argmax().item()) if count else -1
    return out


def compare_hits(torch, got_begin, got_filter, want_begin, want_filter):
    """probe_fanout_hits' arrays against expected_hits': {begin_bad, begin_first, filter_bad, filter_first}."""
    return compare_where_they_live(torch, begin=(got_begin, want_begin), filter=(got_filter, want_filter))


def compare_plan(torch, got, want):
    """(group_table, group_begin, entry_key) against torch_plan's: {table_*, begin_*, key_*}."""
    return compare_where_they_live(torch, table=(got[0], want[0]), begin=(got[1], want[1]), key=(got[2], want[2]))


def assert_same(cmp, what):
    bad = {k[:-4]: (v, cmp[k[:-4] + "_first"]) for k, v in cmp.items() if k.endswith("_bad") and v}
    assert not bad, f"{what}: (entries that differ, the first at) {bad}"
