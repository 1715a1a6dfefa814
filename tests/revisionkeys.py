"""Revisions the revision tests share (tests/test_revision_cpu.py,
tests/test_gpu_revision.py): lists of tests/test_gpu_level_index.py's level
shapes in Revision::Get's visiting order, a lookup pool aimed at the boundaries
of all of them, and the expected candidate lists -- oracle.level_candidates per
level, concatenated level 0 first, shifted to global table ids."""
import numpy as np

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
        _tables[name] = _level(name)
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
