"""GPU: the segmented build's fallback shapes at their seams.

Keys that are not aligned 16-byte keys reach the generic pass A
(bloom_bin_kernel) with any k other than 6, with
ADL_BLOOM_SKIP_ADJACENT_DUPLICATES, from an unaligned buffer and with a fixed
stride.  A route for these shapes through hash pairs in key order
(hash_pairs_device, then bloom_bin_kernel<KeysPair>) was built and measured
("Other key shapes"; profiles/fallback_pairs/); these cases were
written for the seams such a route has, and hold for whatever hashes the keys:

  * a first filter that does not start at key 0, and an empty filter;
  * a duplicate across a 256-key pass-A chunk and a 512-key hashing run, and
    across a filter boundary (the first key of a filter is never skipped);
  * no key at all;
  * more than 8 filters (descriptors in the workspace's FilterTable);
  * every launch runs on the build's stream.

Shapes: variable-length keys of 0..40 bytes in a 16-byte-aligned buffer and one
byte past, and 24-byte keys from key 5 (8 bytes past a 16-byte boundary) and
from key 6 (aligned).  Everything is compared exactly with the oracle over all
keys, duplicates included; outputs and workspaces have the header's exact sizes
inside guard bands, the key buffer and offsets are surrounded by 0xFF bytes
(tests/guardband.py).
"""
import ctypes

import numpy as np
import pytest

import streamorder as so
from guardband import Guarded, Poisoned, check_all

pytestmark = pytest.mark.gpu

SKIP_DUP = 1
NKEYS = 3800  # keys in every buffer; no case uses them all
STRIDE = 24
MODES = [(3, 0), (20, 0), (10, SKIP_DUP)]
MODE_IDS = ["bpk3", "bpk20", "bpk10-skip"]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield torch
    so.release_delay()


@pytest.fixture(scope="module")
def ab():
    import adlbloom

    adlbloom.lib()
    return adlbloom


class KeySet:
    """NKEYS keys, variable-length (0..40 bytes) or of STRIDE bytes; key i
    repeats key i - 1 for every i in `equal` and for every third i if
    `thirds`.  Never modified."""

    def __init__(self, seed, var, equal=(), thirds=False):
        rng = np.random.default_rng(seed)
        lens = rng.integers(0, 41, NKEYS) if var else np.full(NKEYS, STRIDE)
        keys = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
        for i in range(1, NKEYS):
            if i in equal or (thirds and i % 3 == 2):
                keys[i] = keys[i - 1]
        self.var = var
        self.data = np.frombuffer(b"".join(keys), np.uint8)
        self.offs = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
        self._dev, self._want = {}, {}

    def device(self, shift):
        """(keys address `shift` bytes past a 16-byte boundary, offsets address or None, stride)"""
        if shift not in self._dev:
            self._dev[shift] = (Poisoned(self.data, 16, skew=shift), Poisoned(self.offs, 8) if self.var else None)
        dk, do = self._dev[shift]
        return dk.ptr, (do.ptr if do else None), (0 if self.var else STRIDE)

    def want(self, oracle, a, b, bpk):
        """the oracle's bitmap of keys [a, b), computed once"""
        if (a, b, bpk) not in self._want:
            if self.var:
                bm = oracle.keys2block(self.data, self.offs[a:b + 1], bits_per_key=bpk)
            else:
                bm = oracle.keys2block(self.data.reshape(NKEYS, STRIDE)[a:b], bits_per_key=bpk)
            self._want[(a, b, bpk)] = bm
        return self._want[(a, b, bpk)]


_sets = {}
EDGES = (256, 300, 512)  # keys 255 = 256 and 511 = 512 (chunk and run boundaries), 299 = 300


def keyset(var, thirds=False):
    key = (var, thirds)
    if key not in _sets:
        _sets[key] = KeySet(0xFA + 2 * var + thirds, var, equal=EDGES, thirds=thirds)
    return _sets[key]


SHAPES = {"var": (True, 0), "var-shifted": (True, 1), "stride24": (False, 0)}


def build(dev, ab, oracle, S, shift, kb, bpk, flags):
    """adl_bloom_build_segmented_device_ex over filters kb of key set S; exact
    sizes in guard bands; every filter compared with the oracle's bitmap.
    Returns the filters' bitmaps as built."""
    L = ab.lib()
    kb = np.ascontiguousarray(kb, dtype=np.uint64)
    F = len(kb) - 1
    cnt = np.ascontiguousarray(np.diff(kb.astype(np.int64)), dtype=np.uint64)
    nb = [L.adl_bloom_bitmap_bytes(int(c), bpk) for c in cnt]
    alloc = [L.adl_bloom_bitmap_alloc_bytes(int(c), bpk) for c in cnt]
    off = np.concatenate([[0], np.cumsum(alloc)[:-1]]).astype(np.uint64)
    wsb = L.adl_bloom_build_workspace_bytes(cnt.ctypes.data, F, bpk)
    out = Guarded(sum(alloc), 16, name="d_bitmaps")
    ws = Guarded(wsb, 256, name="d_workspace")
    pk, po, stride = S.device(shift)
    rc = L.adl_bloom_build_segmented_device_ex(pk, po, stride, kb.ctypes.data, F, bpk, out.ptr, off.ctypes.data, flags,
                                               ws.ptr, wsb, ab._stream())
    assert rc == 0, rc
    dev.cuda.synchronize()  # (raises if a launch failed)
    got = out.numpy()
    built = []
    for f in range(F):
        want = S.want(oracle, int(kb[f]), int(kb[f + 1]), bpk)
        assert want.size == nb[f]
        g = got[int(off[f]):int(off[f]) + alloc[f]]
        bad = np.nonzero(g[:nb[f]] != want)[0]
        assert bad.size == 0, f"filter {f} {kb[f]}..{kb[f + 1]}: {bad.size} bytes differ, first at {bad[0]}"
        assert not g[nb[f]:].any(), f"filter {f}: the pad bytes are written as zero"
        built.append(g[:nb[f]])
    check_all(out, ws)
    return built


# ---------------------------------------------------------------- a first filter past key 0, an empty filter
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape,first", [("var", 5), ("var-shifted", 5), ("stride24", 5), ("stride24", 6)],
                         ids=["var", "var-shifted", "stride24-from5", "stride24-from6"])
def test_first_filter_past_key_0_and_an_empty_filter(dev, ab, oracle, shape, first, mode):
    var, shift = SHAPES[shape]
    bpk, flags = mode
    build(dev, ab, oracle, keyset(var, thirds=bool(flags)), shift, [first, 300, 300, 1029], bpk, flags)


# ---------------------------------------------------------------- duplicates across chunk, run and filter boundaries
@pytest.mark.parametrize("mode", MODES[1:], ids=MODE_IDS[1:])
@pytest.mark.parametrize("split", [False, True], ids=["one-filter", "boundary-between-equal-keys"])
@pytest.mark.parametrize("n", [511, 512, 513, 1025])
@pytest.mark.parametrize("shape", ["var", "stride24"])
def test_duplicates_across_chunk_and_run_boundaries(dev, ab, oracle, knobs, shape, n, split, mode):
    """ADL_BLOOM_CHUNK_KEYS=256: keys 255 and 256 sit in two pass-A chunks, keys
    511 and 512 in two chunks (and in two 512-key runs of a run hasher); split:
    filter 1 starts at key 256, whose predecessor is equal and belongs to
    filter 0."""
    knobs.set("ADL_BLOOM_CHUNK_KEYS", "256")
    var, shift = SHAPES[shape]
    bpk, flags = mode
    S = keyset(var)
    assert S.offs[256] - S.offs[255] == S.offs[257] - S.offs[256]
    build(dev, ab, oracle, S, shift, [0, 256, n] if split else [0, n], bpk, flags)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_first_key_of_a_filter_is_never_skipped(dev, ab, oracle, shape):
    """Filter 1 is key 300 alone, equal to key 299, the last of filter 0: its
    bitmap is the oracle's (build compares it), not the empty one that
    skipping the key would leave."""
    var, shift = SHAPES[shape]
    S = keyset(var)
    a, b = int(S.offs[299]), int(S.offs[300])
    assert bytes(S.data[a:b]) == bytes(S.data[b:int(S.offs[301])])
    built = build(dev, ab, oracle, S, shift, [0, 300, 301, 600], 10, SKIP_DUP)
    assert built[1].any()


# ---------------------------------------------------------------- no key at all
@pytest.mark.parametrize("shape", ["var", "stride24"])
def test_every_filter_empty(dev, ab, oracle, shape):
    var, shift = SHAPES[shape]
    build(dev, ab, oracle, keyset(var), shift, [7, 7, 7, 7], 3, 0)


# ---------------------------------------------------------------- descriptors in the FilterTable
def test_ten_filters_skip_adjacent_duplicates(dev, ab, oracle):
    """More than 8 filters: fill_maps_kernel and Filt<true>; every third key
    repeats the one before it."""
    sizes = [100, 700, 250, 400, 130, 640, 310, 170, 550, 480]
    kb = 3 + np.concatenate([[0], np.cumsum(sizes)])
    assert len(sizes) == 10 and kb[-1] <= NKEYS
    for shape in ("var", "var-shifted"):
        var, shift = SHAPES[shape]
        build(dev, ab, oracle, keyset(var, thirds=True), shift, kb, 10, SKIP_DUP)


# ---------------------------------------------------------------- the build's stream
def test_every_launch_is_on_the_builds_stream(dev, ab, oracle):
    """The build behind a delay on a non-blocking stream, the keys arriving on
    that stream after the delay (before: a decoy of the same lengths in reverse
    order and other bytes, with no repeated key), then
    adl_bloom_build_positions on that stream with no synchronise in between.
    A launch that reads keys on any other stream reads the decoy: another
    bitmap, and k positions for every key instead of k for every key that
    differs from its predecessor (here: in both hashes, which no two different
    adjacent keys of the set share)."""
    L = ab.lib()
    S = keyset(True, thirds=True)
    n, bpk = 1000, 10
    data, offs = S.data[:int(S.offs[n])], S.offs[:n + 1]
    rng = np.random.default_rng(7)
    ddata = rng.integers(0, 256, data.size, dtype=np.uint8)
    lens = np.diff(offs.astype(np.int64))
    doffs = np.concatenate([[0], np.cumsum(lens[::-1])]).astype(np.uint64)
    pairs = oracle.murmur3_batch(data, offs)
    skipped = int((pairs[1:] == pairs[:-1]).all(1).sum())
    same = sum(bytes(data[offs[i - 1]:offs[i]]) == bytes(data[offs[i]:offs[i + 1]]) for i in range(1, n))
    assert skipped == same >= n // 3  # equal keys and equal pairs are the same keys here
    want_pos = ab.num_probes(bpk) * (n - skipped)
    cnt = np.array([n], np.uint64)
    kb = np.array([0, n], np.uint64)
    boff = np.zeros(1, np.uint64)
    nbytes, alloc = ab.bitmap_bytes(n, bpk), ab.bitmap_alloc_bytes(n, bpk)
    wsb = ab.workspace_bytes([n], bpk)
    case = so.Case()
    keys, d_offs = case.input(data, ddata, pad=32), case.input(offs, doffs)
    bm, ws = case.output(alloc), case.workspace(wsb)
    got_pos = ctypes.c_uint64()

    def entry(s):
        rc = L.adl_bloom_build_segmented_device_ex(keys.data_ptr(), d_offs.data_ptr(), 0, kb.ctypes.data, 1, bpk,
                                                   bm.data_ptr(), boff.ctypes.data, SKIP_DUP, ws.data_ptr(), wsb,
                                                   so.sptr(s))
        assert rc == 0, rc
        rc = L.adl_bloom_build_positions(cnt.ctypes.data, 1, bpk, ws.data_ptr(), ctypes.byref(got_pos), so.sptr(s))
        assert rc == 0, rc

    case.run(entry)
    print(f"positions {got_pos.value}, want {want_pos} ({n} keys, {skipped} skipped)")
    assert got_pos.value == want_pos
    so.check(case.result(bm)[:nbytes], S.want(oracle, 0, n, bpk), "bitmap")
