"""GPU: keys of 4 KiB to 64 KiB and more.

Three length limits of the variable-length build lie above the longest key any
other test uses (700 bytes), and every case here crosses them on purpose:

  * hash_var_kernel keeps lengths in 16 bits (0xffff: "64 KiB or more, re-read
    the offsets and hash from global memory") and sorts into 512 exact-length
    bins, bin 511 meaning "longer";
  * bloom_bin_kernel<KeysVar> stages keys through at most 4 LDS windows; keys
    longer than min(4096, wcap / 2) or starting past the fourth window are
    hashed from global memory;
  * KeysVar::same_as_prev (adjacent-duplicate skipping) compares byte by byte.

One key set, built once and never modified: 3000 keys of random bytes, lengths
log-uniform on 0..8192, among them one key of every length in 509..514,
4090..4100 and 65533..65538 and four keys of 70 001 bytes.  The longest keys
are the first key, the last key and keys 511, 512 and 513 (the hashing pass's
512-key run boundary).  Its first 300 keys (the 70 001-byte key 0 among them)
give one pass-A chunk many times the bytes of its four windows.  The set is
built as one filter and as nine ([0, 1, 511, 512, 513, 2, 300, 1000, rest]
keys; the prefix, which has too few keys for that list, as
[0, 1, 51, 52, 53, 2, 30, 100, rest]).  For adjacent-duplicate skipping every
key of 65 533 bytes or more is doubled, and a filter boundary that follows
such a key falls between its two copies.

Everything is compared exactly with the oracle; outputs and workspaces have
the header's exact sizes inside guard bands (tests/guardband.py), the key
buffer and offsets are surrounded by 0xFF bytes.
"""
import ctypes
import re

import numpy as np
import pytest

from guardband import Guarded, Poisoned, check_all

pytestmark = pytest.mark.gpu

BITMAP_TAIL = 256 << 10
SKIP_DUP, VERIFY = 1, 2
N, PREFIX = 3000, 300
SPLIT9 = {N: [0, 1, 511, 512, 513, 2, 300, 1000], PREFIX: [0, 1, 51, 52, 53, 2, 30, 100]}  # + the rest


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


def make_lengths(seed):
    """N lengths: the explicit ones at their places, the rest log-uniform on 0..8192."""
    rng = np.random.default_rng(seed)
    edge = list(range(509, 515)) + list(range(4090, 4101)) + [65533, 65534, 65535, 65537, 65538]
    lens = np.floor(np.exp(rng.random(N) * np.log(8193.0))).astype(np.int64) - 1
    assert lens.min() >= 0 and lens.max() <= 8192
    fixed = {0: 70_001, 511: 70_001, 512: 65_536, 513: 70_001, N - 1: 70_001}
    free = [i for i in rng.permutation(N) if int(i) not in fixed]
    for i, L in zip(free, edge):
        lens[i] = L
    for i, L in fixed.items():
        lens[i] = L
    return lens


class KeySet:
    def __init__(self, seed, double_long=False):
        lens = make_lengths(seed)
        rng = np.random.default_rng(seed + 1)
        o = np.concatenate([[0], np.cumsum(lens)])
        data = rng.integers(0, 256, int(o[-1]), dtype=np.uint8)
        self.doubled = None
        if double_long:
            # every key of 64 KiB - 3 or more twice in a row; `doubled` maps key i of the plain set
            # to its (first) index here
            parts, new_lens, self.doubled = [], [], np.zeros(N + 1, np.int64)
            for i in range(N):
                self.doubled[i] = len(new_lens)
                for _ in range(2 if lens[i] >= 65_533 else 1):
                    parts.append(data[o[i]:o[i + 1]])
                    new_lens.append(lens[i])
            self.doubled[N] = len(new_lens)
            data, lens = np.concatenate(parts), np.array(new_lens)
        self.data, self.lens, self.n = data, lens, len(lens)
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self._dev = {}

    def device(self, shift):
        """(keys address at `shift` bytes past a 16-byte boundary, offsets address)"""
        if shift not in self._dev:
            self._dev[shift] = (Poisoned(self.data, 16, skew=shift), Poisoned(self.offs, 8))
        dk, do = self._dev[shift]
        return dk.ptr, do.ptr

    def key_begin(self, prefix, nine):
        """key_begin of the first `prefix` keys of the plain set as one filter or as nine"""
        kb = np.concatenate([[0], np.cumsum(SPLIT9[prefix]), [prefix]]) if nine else np.array([0, prefix])
        if self.doubled is not None:
            # a filter boundary after a long key falls between its two copies
            d = self.doubled
            kb = np.array([d[b] - (1 if 0 < b < prefix and d[b] - d[b - 1] == 2 else 0) for b in kb])
        return kb.astype(np.uint64)


_sets = {}


def keyset(name):
    if name not in _sets:
        _sets[name] = {"plain": lambda: KeySet(0x4B), "doubled": lambda: KeySet(0x4B, double_long=True),
                       "fresh": lambda: KeySet(0x7A)}[name]()
    return _sets[name]


_want = {}


def oracle_bitmaps(oracle, name, kb, bpk):
    key = (name, tuple(int(x) for x in kb), bpk)
    if key not in _want:
        S = keyset(name)
        _want[key] = [oracle.keys2block(S.data, S.offs[int(kb[f]):int(kb[f + 1]) + 1], bits_per_key=bpk)
                      for f in range(len(kb) - 1)]
    return _want[key]


def sync(dev):
    dev.cuda.current_stream().synchronize()


def test_key_set_shape():
    S, D = keyset("plain"), keyset("doubled")
    assert S.n == N and [int(S.lens[i]) for i in (0, 511, 512, 513, N - 1)] == [70_001, 70_001, 65_536, 70_001, 70_001]
    for L in list(range(509, 515)) + list(range(4090, 4101)) + list(range(65_533, 65_539)):
        assert (S.lens == L).any(), L
    assert (S.lens == 70_001).sum() == 4 and (S.lens[:PREFIX] >= 65_536).any()
    assert S.lens[:PREFIX].sum() > 4 * 65_536  # one chunk of 300 keys: many times four LDS windows
    assert D.n == N + 10 and D.lens[0] == D.lens[1] == 70_001
    kb = D.key_begin(N, True)
    # key 0 and its copy sit on both sides of the boundary between filters 1 and 2
    assert kb[1] == 0 and kb[2] == 1 and D.lens[1] == 70_001 and kb[-1] == D.n
    assert (np.diff(kb.astype(np.int64)) >= 0).all()


def build(dev, ab, oracle, name, prefix, nine, bpk, shift, flags=0):
    """One filter through adl_bloom_build_device (flags 0) or nine / flagged
    through adl_bloom_build_segmented_device_ex, exact sizes in guard bands."""
    L, S = ab.lib(), keyset(name)
    kb = S.key_begin(prefix, nine)
    F = len(kb) - 1
    cnt = np.ascontiguousarray(np.diff(kb.astype(np.int64)), dtype=np.uint64)
    nb = [L.adl_bloom_bitmap_bytes(int(c), bpk) for c in cnt]
    alloc = [L.adl_bloom_bitmap_alloc_bytes(int(c), bpk) for c in cnt]
    off = np.concatenate([[0], np.cumsum(alloc)[:-1]]).astype(np.uint64)
    wsb = L.adl_bloom_build_workspace_bytes(cnt.ctypes.data, F, bpk)
    out = Guarded(sum(alloc), 16, tail=BITMAP_TAIL, name="d_bitmaps")
    ws = Guarded(wsb, 256, name="d_workspace")
    pk, po = S.device(shift)
    if F == 1 and not flags:
        rc = L.adl_bloom_build_device(pk, po, int(cnt[0]), 0, bpk, out.ptr, ws.ptr, wsb, ab._stream())
    else:
        rc = L.adl_bloom_build_segmented_device_ex(pk, po, 0, kb.ctypes.data, F, bpk, out.ptr, off.ctypes.data, flags,
                                                   ws.ptr, wsb, ab._stream())
    assert rc == 0, rc
    sync(dev)
    want = np.zeros(sum(alloc), np.uint8)
    for f, bm in enumerate(oracle_bitmaps(oracle, name, kb, bpk)):
        want[int(off[f]):int(off[f]) + nb[f]] = bm
    got = out.numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]}; filter offsets {off.tolist()}"
    check_all(out, ws)


@pytest.mark.parametrize("nine", [False, True], ids=["one-filter", "nine-filters"])
@pytest.mark.parametrize("prefix", [N, PREFIX])
@pytest.mark.parametrize("bpk,shift", [(10, 0), (3, 0), (44, 0), (10, 1)],
                         ids=["hashing-pass-bin16", "windows-k2", "windows-k30", "unaligned-no-staging"])
def test_build_long_keys(dev, ab, oracle, bpk, shift, prefix, nine):
    build(dev, ab, oracle, "plain", prefix, nine, bpk, shift)


@pytest.mark.parametrize("nine", [False, True], ids=["one-filter", "nine-filters"])
@pytest.mark.parametrize("prefix", [N, PREFIX])
def test_build_long_keys_skip_adjacent_duplicates(dev, ab, oracle, prefix, nine):
    """Equal keys of 64 KiB and more in a row, also across a filter boundary
    (where the second copy must be hashed: it is the first key of its filter)."""
    build(dev, ab, oracle, "doubled", prefix, nine, 10, 0, flags=SKIP_DUP)


def test_launch_lines_name_the_intended_kernels(dev, ab, oracle, knobs, capfd):
    """A later change of dispatch cannot quietly move these inputs off the
    paths they are meant for."""
    knobs.set("ADL_BLOOM_DEBUG", "1")
    launch = re.compile(r"adl_bloom launch: pass A (?:queued|static) \((.+?), (?:DT|kernarg)\)")
    capfd.readouterr()
    build(dev, ab, oracle, "plain", N, False, 10, 0)
    assert launch.findall(capfd.readouterr().err) == ["bin16 SrcH dense"]
    build(dev, ab, oracle, "plain", N, False, 3, 0)
    assert launch.findall(capfd.readouterr().err) == ["generic bloom_bin_kernel"]


@pytest.mark.parametrize("shift", [0, 1])
def test_murmur3_long_keys(dev, ab, oracle, shift):
    S = keyset("plain")
    pk, po = S.device(shift)
    out = Guarded(8 * S.n, 4, name="d_out")
    rc = ab.lib().adl_bloom_murmur3_device(pk, po, S.n, 0, ab.SEED1, ab.SEED2, out.ptr, ab._stream())
    assert rc == 0, rc
    sync(dev)
    got = out.numpy().view(np.uint32).reshape(S.n, 2)
    bad = np.nonzero((got != oracle.murmur3_batch(S.data, S.offs)).any(1))[0]
    assert bad.size == 0, f"{bad.size} keys differ, first {bad[0]} of {int(S.lens[bad[0]])} bytes"
    out.check()


@pytest.mark.parametrize("form", ["probe", "fanout"])
@pytest.mark.parametrize("queries", ["plain", "fresh"])
def test_probe_long_keys(dev, ab, oracle, queries, form):
    """The set against its own bitmap (all present) and fresh keys of the same
    length distribution (the oracle's answers)."""
    L, S, Q = ab.lib(), keyset("plain"), keyset(queries)
    bm = oracle_bitmaps(oracle, "plain", np.array([0, N]), 10)[0]
    want = oracle.probe(Q.data, bm, offsets=Q.offs, bits_per_key=10)
    assert want.all() or queries == "fresh"
    dbm = Poisoned(bm, 16)
    pk, po = Q.device(0)
    out = Guarded(Q.n, 8, skew=3, name="d_out")
    if form == "probe":
        rc = L.adl_bloom_probe_device(pk, po, Q.n, 0, 10, dbm.ptr, bm.size, out.ptr, ab._stream())
    else:
        pb = Poisoned(np.arange(Q.n + 1, dtype=np.uint32), 4)
        pf = Poisoned(np.zeros(Q.n, np.uint32), 4)
        beg = Poisoned(np.array([0, bm.size], np.uint64), 8)
        rc = L.adl_bloom_probe_fanout_device(pk, po, Q.n, 0, pb.ptr, pf.ptr, Q.n, 1, dbm.ptr, beg.ptr, None, 10,
                                             out.ptr, ab._stream())
    assert rc == 0, rc
    sync(dev)
    got = out.numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} answers differ, first key {bad[0]} of {int(Q.lens[bad[0]])} bytes"
    out.check()


def test_write_through_verify_long_keys(dev, ab, oracle):
    """adl_bloom_filter_cache_build from host keys with ADL_BLOOM_CACHE_VERIFY on
    the 9-filter shape: no key missing, the oracle's block."""
    L, S = ab.lib(), keyset("plain")
    kb = S.key_begin(N, True)
    F = len(kb) - 1
    bms = oracle_bitmaps(oracle, "plain", kb, 10)
    nbytes = L.adl_bloom_filter_block_bytes(kb.ctypes.data, F, 10)
    hb = Guarded(nbytes, 1, device="cpu", name="h_block")
    hk = np.concatenate([np.full(64, 0xFF, np.uint8), S.data, np.full(64, 0xFF, np.uint8)])
    cache = ab.FilterCache(8 << 20, max_tables=8)
    h = ctypes.c_void_p()
    rc = L.adl_bloom_filter_cache_build(cache._h, hk.ctypes.data + 64, S.offs.ctypes.data, 0, kb.ctypes.data, F, 10,
                                        VERIFY, hb.ptr, nbytes, ctypes.byref(h), None)
    assert rc == 0, rc  # a missing key is ADL_FILTER_BLOCK_ERROR (13)
    assert L.adl_bloom_filter_cache_abandon(cache._h, h) == 0
    assert hb.numpy().tobytes() == oracle.filter_block_final([b.tobytes() for b in bms], 10)
    hb.check()
    cache.close()
    boff = np.concatenate([[0], np.cumsum([b.size for b in bms])]).astype(np.uint64)
    assert ab.verify(hk[64:64 + S.data.size], kb, np.concatenate(bms), boff, offsets=S.offs) == (0, None)
