"""The cases of tests/golden/filter_block_ref.json: inputs, and the calls into
the compiled reference (oracle/_ref/libref_filter_block.so) that answer them.

Shared by tests/golden/make_filter_block_ref.py (which records the reference's
answers), tests/test_oracle_reference_cpu.py and tests/test_gpu_reference.py
(which regenerate the inputs, prove by SHA-256 that they are the recorded ones,
and compare).  Nothing here computes a bloom filter: inputs are plain numpy,
answers come from the reference library alone.
"""
import hashlib
import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
JSON_PATH = os.path.join(HERE, "golden", "filter_block_ref.json")

BPKS = (0, 1, 2, 3, 5, 9, 10, 11, 16, 20, 30, 43, 44, 50, 100)
NS = (0, 1, 2, 63, 64, 65, 6145, 50_001)
SHAPES = ("split16", "varlen", "ascii")
# beside the grid: 24-byte keys (the fixed-stride build that is neither 16-byte nor var-len)
EXTRA_BUILDS = (("fixed24", 10, 6145), ("fixed24", 3, 6145))
NMAX = max(NS)
MIN_QUERIES = 1000


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


def load_json():
    with open(JSON_PATH) as f:
        return json.load(f)


# ---------------------------------------------------------------- inputs
class Keys:
    """Packed keys: data (uint8, 16 spare bytes), offs (uint64, n+1)."""

    def __init__(self, data, offs):
        self.offs = np.ascontiguousarray(offs, dtype=np.uint64)
        total = int(self.offs[-1])
        self.data = np.zeros(total + 16, dtype=np.uint8)
        self.data[:total] = data[:total]
        self.n = len(self.offs) - 1

    def head(self, n):
        return self.slice(0, n)

    def slice(self, a, b):
        o = self.offs[a:b + 1]
        return Keys(self.data[int(o[0]):int(o[-1])], o - o[0])

    def key(self, i) -> bytes:
        return self.data[int(self.offs[i]):int(self.offs[i + 1])].tobytes()

    def packed(self) -> bytes:
        return self.data[:int(self.offs[-1])].tobytes()

    def sha(self) -> str:
        """SHA-256 over the offsets (LE u64) and the packed bytes."""
        return sha(self.offs.astype("<u8").tobytes() + self.packed())

    def fixed(self, stride):
        """(n, stride) view of equal-length keys"""
        assert self.n == 0 or (np.diff(self.offs.astype(np.int64)) == stride).all()
        return self.data[:self.n * stride].reshape(self.n, stride)


def cat(*ks):
    offs, base = [np.zeros(1, np.uint64)], 0
    for k in ks:
        offs.append(k.offs[1:] + np.uint64(base))
        base += int(k.offs[-1])
    return Keys(np.concatenate([k.data[:int(k.offs[-1])] for k in ks] + [np.zeros(0, np.uint8)]),
                np.concatenate(offs))


def from_list(keys):
    offs = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
    return Keys(np.frombuffer(b"".join(keys), dtype=np.uint8), offs)


def splitmix16(seed, n, skip=0):
    """SplitMix64 16-byte keys, key i = LE64(next) || LE64(next), in numpy."""
    g = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(2 * skip + 1, 2 * (skip + n) + 1, dtype=np.uint64)) * g
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return Keys(z.astype("<u8").view(np.uint8), np.arange(n + 1, dtype=np.uint64) * np.uint64(16))


def random_varlen(seed, n, lo, hi):
    """n keys of lo..hi random bytes (about half of them >= 0x80)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return Keys(rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8), offs)


def ascii_keys(first, n):
    return from_list([b"key-%d" % i for i in range(first, first + n)])


_streams = {}


def members(shape, n) -> Keys:
    """The first n keys of the shape's member stream."""
    if shape not in _streams:
        _streams[shape] = {"split16": lambda: splitmix16(0x5EED, NMAX),
                           "varlen": lambda: random_varlen(0xB10C, NMAX, 0, 69),
                           "ascii": lambda: ascii_keys(0, NMAX),
                           "fixed24": lambda: random_varlen(0xB10E, 6145, 24, 24)}[shape]()
    return _streams[shape].head(n)


def queries(shape, n) -> Keys:
    """max(n, 1000) keys none of which is a member (the generator checks that)."""
    q = max(n, MIN_QUERIES)
    key = ("q", shape)
    if key not in _streams:
        _streams[key] = {"split16": lambda: splitmix16(0x5EED, NMAX, skip=1_000_000),
                         "varlen": lambda: random_varlen(0xB10D, NMAX, 4, 69),
                         "ascii": lambda: ascii_keys(1_000_000, NMAX),
                         "fixed24": lambda: random_varlen(0xB10F, 6145, 24, 24)}[shape]()
    return _streams[key].head(q)


def all_builds():
    return [(s, b, n) for s in SHAPES for b in BPKS for n in NS] + list(EXTRA_BUILDS)


def build_id(shape, bpk, n):
    return f"{shape}/bpk{bpk}/n{n}"


# ---------------------------------------------------------------- multi-filter blocks
EMPTIES = [0, 0, 5, 0, 0, 17, 1, 0]  # empty filters first, last and adjacent
C70 = [(i * 37) % 211 if i % 9 else 0 for i in range(70)]  # 70 filters of 0..210 keys, eight of them empty
BLOCKS = {
    # name: (key shape, bits_per_key, keys per filter)
    "f1-b10-var": ("varlen", 10, [300]),
    "f1-b1-s16": ("split16", 1, [65]),
    "f1-b44-ascii": ("ascii", 44, [1000]),
    "empties-b1-var": ("varlen", 1, EMPTIES),
    "empties-b10-s16": ("split16", 10, EMPTIES),
    "empties-b10-var": ("varlen", 10, EMPTIES),
    "empties-b44-var": ("varlen", 44, EMPTIES),
    "all-empty-b10": ("split16", 10, [0, 0, 0]),
    "f70-b10-s16": ("split16", 10, C70),
    "f70-b44-var": ("varlen", 44, C70),
    "f10-b10-var50001": ("varlen", 10, [5000] * 9 + [5001]),
}
PER_ID = 24  # members and non-members asked of each filter id


def block_keys(name) -> Keys:
    shape, _, counts = BLOCKS[name]
    return members(shape, sum(counts))


def block_queries(name):
    """(filter ids int32, Keys): for each id 0..F+1 up to PER_ID of that filter's own keys (ids < F) and
    PER_ID non-members (ids 2j and 2j+1 are asked about the same non-members: one key, two filters)."""
    shape, _, counts = BLOCKS[name]
    F = len(counts)
    kb = np.concatenate([[0], np.cumsum(counts)])
    mem, non = members(shape, int(kb[-1])), queries(shape, 0)
    ids, parts = [], []
    for f in range(F + 2):
        if f < F:
            c = min(counts[f], PER_ID)
            parts.append(mem.slice(int(kb[f]), int(kb[f]) + c))
            ids += [f] * c
        a = (f // 2 * PER_ID) % (MIN_QUERIES - PER_ID)
        parts.append(non.slice(a, a + PER_ID))
        ids += [f] * PER_ID
    return np.array(ids, dtype=np.int32), cat(*parts)


BINNED_BLOCK = "f70-b10-s16"
BINNED_N = (1 << 20) + 777


def binned_queries():
    """(filter ids int32, (n,16) keys) of the binned batch probe's case: even queries a key of the
    block with its own filter's id, odd ones a fresh key with any id of 0..F-1."""
    _, _, counts = BLOCKS[BINNED_BLOCK]
    F, total = len(counts), sum(counts)
    owner = np.repeat(np.arange(F), counts)
    rng = np.random.default_rng(0xB177ED)
    pick = rng.integers(0, total, size=BINNED_N)
    fid = rng.integers(0, F, size=BINNED_N).astype(np.int32)
    keys = splitmix16(0x5EED, BINNED_N, skip=2_000_000).fixed(16).copy()
    even = np.arange(BINNED_N) % 2 == 0
    keys[even] = block_keys(BINNED_BLOCK).fixed(16)[pick[even]]
    fid[even] = owner[pick[even]]
    return fid, keys


def split_block(block: bytes):
    """(bitmap bytes per filter, offsets F+1) of a well-formed block, read from its trailer."""
    L = len(block)
    assert block[L - 11:L - 8] == b"bf:" and block[L - 4:] == struct.pack("<i", 7)
    F, start = struct.unpack_from("<i", block, L - 15)[0], struct.unpack_from("<i", block, L - 19)[0]
    assert start + 4 * F == L - 19
    off = list(struct.unpack_from(f"<{F}i", block, start)) + [start]
    return [block[off[f]:off[f + 1]] for f in range(F)], np.array(off, dtype=np.uint64)


# ---------------------------------------------------------------- trailer mutations
def base3():
    """The 3-filter block the mutations start from: filters 0 and 1 are those of the reference's
    test/filter_block_test.cpp:9-29, filter 2 is added.  -> (Keys, counts)"""
    b0 = [b"hello", b"world", b"hello-yly", b"hello-ddl"] + [b"hello-ddl%d" % i for i in range(10000)]
    b1 = [b"adl", b"dont", b"like-apple"]
    b2 = [b"third-%d" % i for i in range(20)]
    return from_list(b0 + b1 + b2), [len(b0), len(b1), len(b2)]


BASE3_BPK = 10
MUT_IDS = (0, 1, 2, 3, 4, 5, 999, 1000, 1001)
MUT_KEYS = (b"hello", b"hello-ddl77", b"adl", b"third-3", b"zackboge", b"dont like-apple")


def mutations(block: bytes):
    """name -> mutated block.  Trailer of the well-formed block of length L: off_0..off_2 at L-31,
    offsets_start at L-19, F at L-15, "bf:" at L-11, bits_per_key at L-8, info_len at L-4."""
    L = len(block)
    (true_start,) = struct.unpack_from("<i", block, L - 19)
    assert true_start == L - 31 and block[L - 11:L - 8] == b"bf:"
    off = [struct.unpack_from("<i", block, L - 31 + 4 * i)[0] for i in range(3)]

    def put(at, v):
        return block[:at] + struct.pack("<i", v) + block[at + 4:]

    out = {}
    for name, v in (("-1", -1), ("0", 0), ("1", 1), ("2", 2), ("6", 6), ("7", 7), ("8", 8), ("len-4", L - 4),
                    ("len-3", L - 3), ("len", L)):
        out["info_len=" + name] = put(L - 4, v)
    out["type[0]"] = block[:L - 11] + b"c" + block[L - 10:]
    out["type[1]"] = block[:L - 10] + b"g" + block[L - 9:]
    for v in (-5, 0, 1, 44, 2**31 - 1):
        out[f"bpk={v}"] = put(L - 8, v)
    for v in (-1, 0, 2, 3, 4, 1000):
        out[f"F={v}"] = put(L - 15, v)
    for name, v in (("-1", -1), ("0", 0), ("4", 4), ("true-4", true_start - 4), ("true+4", true_start + 4),
                    ("len", L), ("2^31-1", 2**31 - 1)):
        out["offsets_start=" + name] = put(L - 19, v)
    out["off_0=1"] = put(L - 31, 1)
    out["off_1>off_2"] = put(L - 27, off[2] + 1)
    out["off_2>offsets_start"] = put(L - 23, true_start + 1)
    for t in (1, 3, 4, 11):
        out[f"truncate-{t}"] = block[:L - t]
    return out


# ---------------------------------------------------------------- the compiled reference
FILTER_BLOCK_ERROR = 13
REF_OUTSIDE, REF_DIV_ZERO = -1, -2
CODE = {0: "0", 1: "1", REF_OUTSIDE: "o", REF_DIV_ZERO: "z"}


class Ref:
    """Calls into oracle/_ref/libref_filter_block.so (R: oracle.ref_filter_block_lib())."""

    def __init__(self, R):
        self.R = R
        assert R.ref_code_outside() == REF_OUTSIDE and R.ref_code_div_zero() == REF_DIV_ZERO

    def keys2block(self, bpk, k: Keys) -> bytes:
        cap = (k.n * max(bpk, 0) + 7) + 64
        out = np.empty(cap, dtype=np.uint8)
        n = self.R.ref_keys2block(bpk, k.data.ctypes.data, k.offs.ctypes.data, k.n, out.ctypes.data, cap)
        assert n >= 0
        return out[:n].tobytes()

    def probe(self, bpk, k: Keys, bitmap: bytes) -> np.ndarray:
        bm = np.frombuffer(bitmap, dtype=np.uint8)
        out = np.empty(max(k.n, 1), dtype=np.uint8)
        rc = self.R.ref_is_key_exists_batch(bpk, k.data.ctypes.data, k.offs.ctypes.data, k.n, bm.ctypes.data, bm.size,
                                            out.ctypes.data)
        assert rc == 0
        return out[:k.n]

    def block(self, bpk, k: Keys, counts) -> bytes:
        cnt = np.ascontiguousarray(counts, dtype=np.uint64)
        assert int(cnt.sum()) == k.n
        cap = sum(int(c) * max(bpk, 0) + 7 for c in counts) + 4 * len(counts) + 64
        out = np.empty(cap, dtype=np.uint8)
        n = self.R.ref_filter_block_build(bpk, k.data.ctypes.data, k.offs.ctypes.data, cnt.ctypes.data, len(cnt),
                                          out.ctypes.data, cap)
        assert n >= 0
        return out[:n].tobytes()

    def reader_init(self, block: bytes) -> int:
        b = np.frombuffer(block + b"\0", dtype=np.uint8)
        return self.R.ref_reader_init(b.ctypes.data, len(block))

    def reader_exists(self, block: bytes, fid: int, key: bytes) -> int:
        b = np.frombuffer(block + b"\0", dtype=np.uint8)
        return self.R.ref_reader_is_key_exists(b.ctypes.data, len(block), fid, key, len(key))

    def reader_probe(self, block: bytes, ids, k: Keys) -> np.ndarray:
        """int8 per query: 0/1, REF_OUTSIDE or REF_DIV_ZERO (Init must succeed)."""
        b = np.frombuffer(block + b"\0", dtype=np.uint8)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        assert len(ids) == k.n
        out = np.empty(max(k.n, 1), dtype=np.int8)
        rc = self.R.ref_reader_is_key_exists_batch(b.ctypes.data, len(block), ids.ctypes.data, k.data.ctypes.data,
                                                   k.offs.ctypes.data, k.n, out.ctypes.data)
        assert rc == 0, rc
        return out[:k.n]

    def mutation(self, block: bytes):
        """(Init's RC or REF_OUTSIDE, one character per (id, key) of MUT_IDS x MUT_KEYS or None)"""
        rc = self.reader_init(block)
        if rc != 0:
            return rc, None
        return rc, "".join(CODE[self.reader_exists(block, i, k)] for i in MUT_IDS for k in MUT_KEYS)


def check_reader_rule(name, g, got_rc, exists, rejected, empty_range):
    """The reader rule for one mutation: g the recorded (or live) reference result {rc, answers},
    got_rc the checked reader's Init, exists(id, key) its IsKeyExists; rejected and empty_range the
    caller's named divergences.  Whatever the reference rejects (or the harness refuses to hand it) the
    checked reader rejects; what the checked reader accepts the reference accepts, and they agree on
    every id; anything else must be listed."""
    if g["rc"] in (FILTER_BLOCK_ERROR, REF_OUTSIDE):
        assert got_rc == FILTER_BLOCK_ERROR
        assert name not in rejected and name not in empty_range
        return
    assert g["rc"] == 0
    if got_rc != 0:
        assert got_rc == FILTER_BLOCK_ERROR
        assert name in rejected, f"unlisted divergence: {name}"
        return
    assert name not in rejected, f"{name} is listed as rejected but was accepted"
    want = g["answers"]
    pairs = [(i, k) for i in MUT_IDS for k in MUT_KEYS]
    assert len(want) == len(pairs)
    assert ("z" in want) == (name in empty_range), f"unlisted divergence: {name}"
    for (i, k), w in zip(pairs, want):
        assert w in "01z", f"{name}: accepted, but the reference would read outside the block for id {i}"
        assert int(exists(i, k)) == (0 if w == "z" else int(w)), (name, i, k)


def bits_hex(answers) -> str:
    return np.packbits(np.asarray(answers, dtype=np.uint8), bitorder="little").tobytes().hex()


def hex_bits(h, n) -> np.ndarray:
    return np.unpackbits(np.frombuffer(bytes.fromhex(h), dtype=np.uint8), bitorder="little")[:n]
