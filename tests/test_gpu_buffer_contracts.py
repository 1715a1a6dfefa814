"""GPU: what a call of include/adl_bloom.h may write.

Every output and workspace here has exactly the size the header promises and
the weakest alignment it grants (bitmaps and d_block 16, workspaces 256, u32 /
u64 arrays their own size, byte outputs 1 -- run at 0, 1 and 3 bytes past an
8-byte boundary), inside a larger tensor filled with 0xA5 (tests/guardband.py).
Each case compares the results exactly with the oracle and then checks that
the bands around every guarded buffer still hold 0xA5.  Bitmap outputs have a
256 KiB tail band: more than one pass-B tile of 128 KiB, so a whole stray tile
store still lands in the band.

Inputs are poisoned the other way: key buffers and offset arrays are preceded
and followed by 0xFF bytes, so equality with the oracle also shows that no
byte outside a key reaches its hash.

Segmented builds place the filters in one guarded buffer in a shuffled order
(no filter in its own slot) with 0xA5 gaps between them, and compare the whole
buffer with an expected image in one comparison: filter f overrunning into a
neighbour that is written later shows as a damaged gap.

Combinations dropped from the segmented build, because they run the same
kernels as a case that is kept:
  * the knob sets (ADL_BLOOM_CLAIM=0, CLAIM=2 + CLAIM_CAP=101,
    BUILD_QUEUES=3) with ADL_BLOOM_SKIP_ADJACENT_DUPLICATES: that flag always
    takes the generic static pass A, which has no claim layout of its own and
    no work-queue form; pass B in the claim layout and from the queues is
    covered by the flag-0 cases;
  * the knob sets with stride-24 keys: stride 24 takes the same generic
    pass A whatever the knobs say, and shares pass B with the 16-byte keys.

NOT tested: reads outside the buffers.  The header's promise that for an
unaligned key buffer "every access stays inside the key bytes" could only be
checked by placing a buffer at the end of an allocation, which can fail only by
faulting the GPU.
"""
import ctypes

import numpy as np
import pytest

from guardband import Guarded, Poisoned, check_all

pytestmark = pytest.mark.gpu

BITMAP_TAIL = 256 << 10
SKIP_DUP, VERIFY = 1, 2
U64_MAX = (1 << 64) - 1


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


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def host_poisoned(a):
    """(numpy holder, address) of a host copy of `a` with 0xFF bytes around it."""
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf = np.full(raw.size + 128, 0xFF, np.uint8)
    buf[64:64 + raw.size] = raw
    return buf, buf.ctypes.data + 64


class Keys:
    """n keys in one of the views `k16`, `k16+1`, `s24`, `var`, `var+1`: the host
    arrays the oracle reads, and poisoned device (and, on demand, host) copies.
    runs: keys repeat in runs (sorted draws with replacement), for the
    adjacent-duplicate flag."""

    def __init__(self, view, n, seed, runs=False):
        rng = np.random.default_rng(seed)
        self.view, self.n = view, n
        skew = 1 if view.endswith("+1") else 0
        idx = np.sort(rng.integers(0, n, n)) if runs and n else np.arange(n)
        if view.startswith("var"):
            lens = rng.integers(0, 91, n)
            o = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            base = rng.integers(0, 256, int(o[-1]), dtype=np.uint8)
            self.stride = 0
            self.h = (np.concatenate([base[o[i]:o[i + 1]] for i in idx]) if n else base).astype(np.uint8)
            self.ho = np.concatenate([[0], np.cumsum(lens[idx])]).astype(np.uint64)
            self.do = Poisoned(self.ho, 8)
        else:
            self.stride = 24 if view == "s24" else 16
            self.h = rng.integers(0, 256, (n, self.stride), dtype=np.uint8)[idx]
            self.ho, self.do = None, None
        self.dk = Poisoned(self.h, 16, skew=skew)
        self.po = None if self.do is None else self.do.ptr

    def part(self, a, b):
        """(keys, offsets) of keys [a, b) for the oracle."""
        if self.ho is None:
            return self.h[a:b], None
        return self.h, self.ho[a:b + 1]

    def host(self):
        """(keys address, offsets address or None) of poisoned host copies."""
        self._hk = host_poisoned(self.h)
        self._ho = None if self.ho is None else host_poisoned(self.ho)
        return self._hk[1], None if self._ho is None else self._ho[1]


def bitmaps_of(oracle, K, kb, bpk):
    return [oracle.keys2block(*K.part(int(kb[f]), int(kb[f + 1])), bits_per_key=bpk) for f in range(len(kb) - 1)]


def sync(dev):
    dev.cuda.current_stream().synchronize()


# ----------------------------------------------------------------- single build
def single_build(dev, ab, oracle, view, n, bpk, nbytes=None):
    L = ab.lib()
    K = Keys(view, n, seed=1000 * n + bpk)
    cnt = u64([n])
    wsb = L.adl_bloom_build_workspace_bytes(cnt.ctypes.data, 1, bpk)
    alloc, nb = L.adl_bloom_bitmap_alloc_bytes(n, bpk), L.adl_bloom_bitmap_bytes(n, bpk)
    assert nb == n * bpk + 7 and alloc == (nb + 15) // 16 * 16 and (nbytes is None or nb == nbytes)
    bm = Guarded(alloc, 16, tail=BITMAP_TAIL, name="d_bitmap")
    ws = Guarded(wsb, 256, name="d_workspace")
    rc = L.adl_bloom_build_device(K.dk.ptr, K.po, n, K.stride, bpk, bm.ptr, ws.ptr, wsb, ab._stream())
    assert rc == 0, rc
    sync(dev)
    want = np.zeros(alloc, np.uint8)
    want[:nb] = oracle.keys2block(*K.part(0, n), bits_per_key=bpk)
    got = bm.numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]} of {nb} (+{alloc - nb} pad)"
    check_all(bm, ws)


VIEWS = ["k16", "k16+1", "s24", "var", "var+1"]


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("n,bpk,nbytes", [(0, 10, 7), (1, 10, 17), (3, 0, 7), (9, 1, 16), (10, 1, 17), (513, 10, 5137),
                                          (6145, 10, 61457), (1000, 44, 44007)])
def test_single_build(dev, ab, oracle, view, n, bpk, nbytes):
    single_build(dev, ab, oracle, view, n, bpk, nbytes)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("n,bpk,nbytes", [(1017, 1, 1024), (1018, 1, 1025), (1000, 10, 10007)])
def test_single_build_128_byte_tiles(dev, ab, oracle, knobs, view, n, bpk, nbytes):
    """ADL_BLOOM_TILE_LOG2=10: exactly 8 tiles, one byte into a 9th, and a
    partial last tile of 32 bytes (10 016 = 78 * 128 + 32)."""
    knobs.set("ADL_BLOOM_TILE_LOG2", 10)
    single_build(dev, ab, oracle, view, n, bpk, nbytes)


# ----------------------------------------------------------------- segmented build
SIZES8 = [300, 0, 1, 1625, 0, 300, 257, 300]
SIZES14 = [0, 1, 511, 512, 513, 1025, 0, 1, 769, 3, 700, 12, 4096, 1]


def shuffled_layout(sizes, seed, device_gaps):
    """Offsets of len(sizes) ranges in one buffer, in a seeded order that leaves
    no range in its own slot.  device_gaps: 16-byte-aligned gaps of 16..4096
    bytes before each range (and after the last); else gaps of 1..40 bytes that
    put every range at an odd offset.  -> (offsets by filter, total bytes)"""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    order = rng.permutation(F)
    while F > 1 and (order == np.arange(F)).any():
        order = rng.permutation(F)
    off, o = np.zeros(F, np.uint64), 0
    for f in order:
        if device_gaps:
            o += 16 * int(rng.integers(1, 257))
        else:
            o += int(rng.integers(1, 40))
            o += 1 - o % 2
        off[f] = o
        o += int(sizes[f])
    o += 16 * int(rng.integers(1, 257)) if device_gaps else int(rng.integers(1, 41))
    return off, o


KNOBSETS = {
    "default": {},
    "claim0": {"ADL_BLOOM_CLAIM": 0},
    "claim2cap101": {"ADL_BLOOM_CLAIM": 2, "ADL_BLOOM_CLAIM_CAP": 101},
    "queues3": {"ADL_BLOOM_BUILD_QUEUES": 3},
}
SEG_CASES = [(v, 0, k) for v in ("k16", "var") for k in KNOBSETS] + [("s24", 0, "default")] + \
            [(v, SKIP_DUP, "default") for v in ("k16", "var", "s24")]


@pytest.mark.parametrize("view,flags,knobset", SEG_CASES)
@pytest.mark.parametrize("sizes", [SIZES8, SIZES14], ids=["8-kernarg", "14-table"])
def test_segmented_build_shuffled_with_gaps(dev, ab, oracle, knobs, sizes, view, flags, knobset):
    for k, v in KNOBSETS[knobset].items():
        knobs.set(k, v)
    L, bpk, F = ab.lib(), 10, len(sizes)
    kb = u64(np.concatenate([[0], np.cumsum(sizes)]))
    K = Keys(view, int(kb[-1]), seed=F, runs=True)
    cnt = u64(sizes)
    nb = [L.adl_bloom_bitmap_bytes(n, bpk) for n in sizes]
    alloc = [L.adl_bloom_bitmap_alloc_bytes(n, bpk) for n in sizes]
    off, total = shuffled_layout(alloc, seed=F + 1, device_gaps=True)
    assert not (off % 16).any()
    wsb = L.adl_bloom_build_workspace_bytes(cnt.ctypes.data, F, bpk)
    out = Guarded(total, 16, tail=BITMAP_TAIL, name="d_bitmaps")
    ws = Guarded(wsb, 256, name="d_workspace")
    rc = L.adl_bloom_build_segmented_device_ex(K.dk.ptr, K.po, K.stride, kb.ctypes.data, F, bpk, out.ptr,
                                               off.ctypes.data, flags, ws.ptr, wsb, ab._stream())
    assert rc == 0, rc
    sync(dev)
    want = np.full(total, 0xA5, np.uint8)
    for f, bm in enumerate(bitmaps_of(oracle, K, kb, bpk)):
        o = int(off[f])
        want[o:o + alloc[f]] = 0
        want[o:o + nb[f]] = bm
    got = out.numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]}; filter offsets {off.tolist()}"
    check_all(out, ws)


# ----------------------------------------------------------------- filter block
def _counts70():
    c = np.random.default_rng(70).integers(0, 18, 70)
    c[10], c[11], c[12] = 0, 1, 0  # 7-byte and 17-byte bitmaps side by side
    return [int(x) for x in c] + [3000]


BLOCK_COUNTS = {"f0": [], "f1_n5": [5], "f1_n1": [1], "f3": [0, 1, 0], "f71": _counts70()}


def test_filter_block_sizes_cover_four_residues(ab):
    res = {ab.filter_block_bytes(np.concatenate([[0], np.cumsum(c)]), 10) % 16 for c in BLOCK_COUNTS.values()}
    assert ab.filter_block_bytes([0], 10) == 19 and len(res) >= 4, sorted(res)


@pytest.mark.parametrize("view", ["k16", "var"])
@pytest.mark.parametrize("name", list(BLOCK_COUNTS))
def test_filter_block_exact_size(dev, ab, oracle, name, view):
    L, bpk, counts = ab.lib(), 10, BLOCK_COUNTS[name]
    F = len(counts)
    kb = u64(np.concatenate([[0], np.cumsum(counts)]))
    K = Keys(view, int(kb[-1]), seed=31 + F)
    nbytes = L.adl_bloom_filter_block_bytes(kb.ctypes.data, F, bpk)
    wsb = L.adl_bloom_filter_block_workspace_bytes(kb.ctypes.data, F, bpk)
    assert nbytes == sum(n * bpk + 7 for n in counts) + 4 * F + 19
    blk = Guarded(nbytes, 16, name="d_block")
    ws = Guarded(wsb, 256, name="d_workspace")
    rc = L.adl_bloom_filter_block_build_device(K.dk.ptr, K.po, K.stride, kb.ctypes.data, F, bpk, blk.ptr, nbytes,
                                               ws.ptr, wsb, ab._stream())
    assert rc == 0, rc
    sync(dev)
    want = oracle.filter_block_final([b.tobytes() for b in bitmaps_of(oracle, K, kb, bpk)], bpk)
    assert blk.numpy().tobytes() == want
    check_all(blk, ws)


# ----------------------------------------------------------------- write-through
def check_resident(ab, oracle, cache, oid, K, kb, bms, bpk):
    """Every filter of the published table answers as the oracle does for its
    own keys and for fresh ones, no query uncached."""
    for f, bm in enumerate(bms):
        a, b = int(kb[f]), int(kb[f + 1])
        fresh = Keys(K.view, 16, seed=7000 + f)
        for member, (keys, offs) in ((True, K.part(a, b)), (False, fresh.part(0, 16))):
            n = len(offs) - 1 if offs is not None else len(keys)
            if n == 0:
                continue
            want = oracle.probe(keys, bm, offsets=offs, bits_per_key=bpk)
            got, unc = cache.probe([oid], np.zeros(n, np.uint32), keys, offsets=offs, filter=f)
            assert unc == 0 and np.array_equal(got, want), f
            assert got.all() or not member


@pytest.mark.parametrize("flags", [0, VERIFY])
@pytest.mark.parametrize("counts", [[1000], [300, 0, 1625]], ids=["one-filter-in-place", "three-filters"])
@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("variant", ["device", "host"])
def test_write_through_build(dev, ab, oracle, variant, pinned, counts, flags):
    L, bpk, F = ab.lib(), 10, len(counts)
    kb = u64(np.concatenate([[0], np.cumsum(counts)]))
    K = Keys("var" if flags else "k16", int(kb[-1]), seed=97 + F)
    nbytes = L.adl_bloom_filter_block_bytes(kb.ctypes.data, F, bpk)
    hb = Guarded(nbytes, 1, pinned_host=pinned, device="cpu", name="h_block")
    cache = ab.FilterCache(8 << 20, max_tables=8)
    h = ctypes.c_void_p()
    guarded = [hb]
    if variant == "device":
        wsb = L.adl_bloom_filter_cache_build_workspace_bytes(kb.ctypes.data, F, bpk)
        ws = Guarded(wsb, 256, name="d_workspace")
        guarded.append(ws)
        rc = L.adl_bloom_filter_cache_build_device(cache._h, K.dk.ptr, K.po, K.stride, kb.ctypes.data, F, bpk, flags,
                                                   ws.ptr, wsb, hb.ptr, nbytes, ctypes.byref(h), ab._stream())
    else:
        pk, po = K.host()
        rc = L.adl_bloom_filter_cache_build(cache._h, pk, po, K.stride, kb.ctypes.data, F, bpk, flags, hb.ptr,
                                            nbytes, ctypes.byref(h), None)
    assert rc == 0, rc
    oid = b"guarded"
    assert L.adl_bloom_filter_cache_publish(cache._h, h, oid, len(oid)) == 0
    sync(dev)
    bms = bitmaps_of(oracle, K, kb, bpk)
    assert hb.numpy().tobytes() == oracle.filter_block_final([b.tobytes() for b in bms], bpk)
    check_all(*guarded)
    check_resident(ab, oracle, cache, oid, K, kb, bms, bpk)
    cache.close()


# ----------------------------------------------------------------- host segmented build
@pytest.mark.parametrize("view", ["k16", "var"])
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_segmented_build_exact_lengths(dev, ab, oracle, pinned, view):
    """Exact-length bitmaps at odd host offsets with gaps of 1 to 40 bytes: a
    download of the 16-byte-rounded device length instead of the exact one
    damages a gap (or the neighbour written before it)."""
    L, bpk = ab.lib(), 10
    sizes = SIZES14 + [120_001]
    F = len(sizes)
    kb = u64(np.concatenate([[0], np.cumsum(sizes)]))
    K = Keys(view, int(kb[-1]), seed=15)
    nb = [L.adl_bloom_bitmap_bytes(n, bpk) for n in sizes]
    off, total = shuffled_layout(nb, seed=16, device_gaps=False)
    assert (off % 2 == 1).all()
    out = Guarded(total, 1, pinned_host=pinned, device="cpu", name="h_bitmaps")
    pk, po = K.host()
    rc = L.adl_bloom_build_segmented(pk, po, K.stride, kb.ctypes.data, F, bpk, out.ptr, off.ctypes.data, None)
    assert rc == 0, rc
    want = np.full(total, 0xA5, np.uint8)
    for f, bm in enumerate(bitmaps_of(oracle, K, kb, bpk)):
        want[int(off[f]):int(off[f]) + nb[f]] = bm
    got = out.numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]}; filter offsets {off.tolist()}"
    out.check()


# ----------------------------------------------------------------- direct probes
class Filters:
    """Bitmaps of 16-byte SplitMix key sets (None: a filter of 0 bytes), packed
    back to back for the oracle, and device arenas that hold them back to back
    or with gaps, surrounded by `bg` bytes."""

    def __init__(self, oracle, counts, bpk, seed0):
        self.counts, self.bpk, self.seed0, self.F = counts, bpk, seed0, len(counts)
        self.bms = [np.zeros(0, np.uint8) if n is None else
                    oracle.keys2block(oracle.splitmix_keys16(seed0 + t, n), bits_per_key=bpk)
                    for t, n in enumerate(counts)]
        self.off = u64(np.concatenate([[0], np.cumsum([b.size for b in self.bms])]))
        self.flat = np.concatenate(self.bms + [np.zeros(1, np.uint8)])

    def queries(self, oracle, n, seed, extra_ids=2):
        """n 16-byte queries: random filter ids (some past the last filter), about
        half of them keys of their filter.  -> (keys, ids, oracle answers)"""
        rng = np.random.default_rng(seed)
        fid = rng.integers(0, self.F + extra_ids, n).astype(np.uint32)
        keys = oracle.splitmix_keys16(seed, n)
        ins = rng.integers(0, 2, n).astype(bool)
        for t in np.unique(fid[ins]):
            c = self.counts[t] if t < self.F else None
            if c:
                sel = np.nonzero(ins & (fid == t))[0]
                keys[sel] = oracle.splitmix_keys16(self.seed0 + int(t), c)[rng.integers(0, c, sel.size)]
        return keys, fid, oracle.probe_multi(keys, fid, self.flat, self.off, bits_per_key=self.bpk)

    def arena(self, dev, bg, gaps):
        """-> (device tensor, begin, end) with `bg` bytes before, between (gaps)
        and after the bitmaps; end[f] == begin[f+1] without gaps."""
        rng = np.random.default_rng(5)
        begin, end, o = [], [], 300
        for b in self.bms:
            if gaps:
                o += int(rng.integers(1, 300))
            begin.append(o)
            o += b.size
            end.append(o)
        host = np.full(o + 300, bg, np.uint8)
        for b, s in zip(self.bms, begin):
            host[s:s + b.size] = b
        return dev.from_numpy(host).cuda(), u64(begin), u64(end)


_cache = {}


def small_filters(oracle):
    if "small" not in _cache:
        _cache["small"] = Filters(oracle, [5000, None, 0, 1, 300], 10, seed0=0xB100)
    return _cache["small"]


def fanout_pairs(n_pairs, seed):
    """Pair lists of 0 to 3 filters per key, n_pairs pairs in all -> pair_begin (u32, keys + 1)."""
    rng = np.random.default_rng(seed)
    per = []
    while sum(per) < n_pairs:
        per.append(min(int(rng.integers(0, 4)), n_pairs - sum(per)))
    per.append(0)  # the last key has no candidate filter
    return np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)


def run_probe(dev, ab, oracle, FL, form, n, skew):
    """One direct-probe entry point, twice: the arena's gaps and surroundings
    all 0x00, then all 0xFF.  The same answers, equal to the oracle's."""
    L, bpk = ab.lib(), FL.bpk
    keys, fid, want = FL.queries(oracle, n, seed=n)
    dk, dfid = Poisoned(keys, 16), Poisoned(fid, 4)
    if form == "fanout":
        pb = fanout_pairs(n, seed=n)
        pair_key = np.repeat(np.arange(len(pb) - 1), np.diff(pb.astype(np.int64)))
        keys_f = oracle.splitmix_keys16(n + 1, len(pb) - 1)
        for i in range(0, len(pb) - 1, 2):  # every other key is a key of its first candidate filter
            t = int(fid[pb[i]]) if pb[i] < pb[i + 1] else FL.F
            if t < FL.F and FL.counts[t]:
                keys_f[i] = oracle.splitmix_keys16(FL.seed0 + t, FL.counts[t])[i % FL.counts[t]]
        # pair p keeps query p's filter id; its key is its owner's
        want = oracle.probe_multi(keys_f[pair_key], fid, FL.flat, FL.off, bits_per_key=bpk)
        dk, dpb = Poisoned(keys_f, 16), Poisoned(pb, 4)
    answers = []
    for bg in (0x00, 0xFF):
        arena, begin, end = FL.arena(dev, bg, gaps=form in ("ranges", "fanout"))
        dbeg = Poisoned(np.concatenate([begin, end[-1:]]), 8)
        dend = Poisoned(end, 8)
        st = ab._stream()
        if form == "single":
            outs = []
            for f in range(FL.F):
                if FL.bms[f].size == 0:
                    continue
                o1 = Guarded(n, 8, skew=skew, name=f"d_out (filter {f})")
                rc = L.adl_bloom_probe_device(dk.ptr, None, n, 16, bpk, arena.data_ptr() + int(begin[f]),
                                              FL.bms[f].size, o1.ptr, st)
                assert rc == 0, rc
                outs.append((f, o1))
            sync(dev)
            for f, o1 in outs:
                assert np.array_equal(o1.numpy(), oracle.probe(keys, FL.bms[f], bits_per_key=bpk)), f
                o1.check()
            answers.append(b"".join(o1.numpy().tobytes() for _, o1 in outs))
            continue
        out = Guarded(n, 8, skew=skew, name="d_out")
        if form == "multi":
            rc = L.adl_bloom_probe_multi_device(dk.ptr, None, n, 16, dfid.ptr, FL.F, arena.data_ptr(), dbeg.ptr, bpk,
                                                out.ptr, st)
        elif form == "ranges":
            rc = L.adl_bloom_probe_ranges_device(dk.ptr, None, n, 16, dfid.ptr, FL.F, arena.data_ptr(), dbeg.ptr,
                                                 dend.ptr, bpk, out.ptr, st)
        else:
            rc = L.adl_bloom_probe_fanout_device(dk.ptr, None, len(pb) - 1, 16, dpb.ptr, dfid.ptr, n, FL.F,
                                                 arena.data_ptr(), dbeg.ptr, dend.ptr, bpk, out.ptr, st)
        assert rc == 0, rc
        sync(dev)
        got = out.numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"bg {bg:#x}: {bad.size} answers differ, first at {bad[0]}"
        out.check()
        answers.append(got.tobytes())
    assert answers[0] == answers[1]


@pytest.mark.parametrize("skew", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("form", ["single", "multi", "ranges", "fanout"])
def test_direct_probes(dev, ab, oracle, form, n, skew):
    run_probe(dev, ab, oracle, small_filters(oracle), form, n, skew)


def test_direct_probe_4097_filters(dev, ab, oracle):
    """More than 4096 filters: no divisor table in LDS."""
    counts = [int(c) for c in np.random.default_rng(4097).integers(0, 41, 4097)]
    FL = Filters(oracle, counts, 10, seed0=0xC000)
    for form in ("multi", "ranges"):
        run_probe(dev, ab, oracle, FL, form, 1000, 3)


# ----------------------------------------------------------------- binned probe
@pytest.mark.parametrize("case", ["9-filters-bpk10", "300-filters-bpk3"])
def test_binned_probe_exact_workspace(dev, ab, oracle, case):
    """pb_bin_kernel<6> (k = 6) and pb_bin_kernel<0> (k = 2) with a workspace of
    exactly adl_bloom_probe_batch_workspace_bytes, pre-filled 0xA5 and then
    0x00: the same answers, the oracle's."""
    L, n = ab.lib(), (1 << 20) + 8195
    if case.startswith("9"):
        counts, bpk = [1, 13, 50_000, None, 120_000, 7, 300_000, 0, 20_000], 10
    else:
        counts, bpk = [int(c) for c in np.random.default_rng(300).integers(0, 20_000, 300)], 3
    FL = Filters(oracle, counts, bpk, seed0=0xD000)
    keys, fid, want = FL.queries(oracle, n, seed=300 + bpk)
    dk, dfid = Poisoned(keys, 16), Poisoned(fid, 4)
    arena, begin, end = FL.arena(dev, 0xFF, gaps=False)
    doff = Poisoned(np.concatenate([begin, end[-1:]]), 8)
    wsb = L.adl_bloom_probe_batch_workspace_bytes(n, FL.F, bpk, 16)
    assert wsb > 0
    answers = []
    for fill in (0xA5, 0x00):
        ws = Guarded(wsb, 256, name="d_workspace")
        ws.view.fill_(fill)
        out = Guarded(n, 8, skew=3, name="d_out")
        rc = L.adl_bloom_probe_batch_device(dk.ptr, None, n, 16, dfid.ptr, FL.F, arena.data_ptr(), doff.ptr, None,
                                            bpk, out.ptr, ws.ptr, wsb, ab._stream())
        assert rc == 0, rc
        sync(dev)
        got = out.numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"workspace fill {fill:#x}: {bad.size} answers differ, first at {bad[0]}"
        check_all(out, ws)
        assert not bool((ws.view == fill).all())  # the binned pipeline ran: the direct kernel has no workspace
        answers.append(got.tobytes())
    assert answers[0] == answers[1]


# ----------------------------------------------------------------- the rest
def test_verify_result_is_16_bytes(dev, ab, oracle):
    L, bpk = ab.lib(), 10
    FL = Filters(oracle, [300, 0, 1625], bpk, seed0=0xE000)
    kb = u64([0, 300, 300, 1925])
    keys = np.concatenate([oracle.splitmix_keys16(0xE000 + t, n) for t, n in enumerate(FL.counts)])
    dk, dkb = Poisoned(keys, 16), Poisoned(kb, 8)
    arena, begin, end = FL.arena(dev, 0xFF, gaps=True)
    dbeg, dend = Poisoned(begin, 8), Poisoned(end, 8)

    def verify():
        res = Guarded(16, 8, name="d_result")
        rc = L.adl_bloom_verify_device(dk.ptr, None, len(keys), 16, dkb.ptr, FL.F, arena.data_ptr(), dbeg.ptr,
                                       dend.ptr, bpk, res.ptr, ab._stream())
        assert rc == 0, rc
        sync(dev)
        res.check()
        return [int(x) for x in res.numpy().view(np.uint64)]

    assert verify() == [0, U64_MAX]
    arena[int(begin[2]):int(end[2])] = 0  # filter 2 loses every bit: its 1625 keys are missing, key 300 first
    assert verify() == [1625, 300]


@pytest.mark.parametrize("seeds", [None, (0, 0x9E3779B9)], ids=["filter-seeds", "other-seeds"])
@pytest.mark.parametrize("view", ["k16", "k16+1", "var", "var+1"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_murmur3_output_is_8n_bytes(dev, ab, oracle, n, view, seeds):
    sa, sb = seeds or (ab.SEED1, ab.SEED2)
    K = Keys(view, n, seed=n)
    out = Guarded(8 * n, 4, name="d_out")
    rc = ab.lib().adl_bloom_murmur3_device(K.dk.ptr, K.po, n, K.stride, sa, sb, out.ptr, ab._stream())
    assert rc == 0, rc
    sync(dev)
    want = oracle.murmur3_batch(*K.part(0, n), seed_a=sa, seed_b=sb)
    assert np.array_equal(out.numpy().view(np.uint32).reshape(n, 2), want)
    out.check()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_synth_keys16_output(dev, ab, oracle, n):
    out = Guarded(16 * n, 16, name="d_out")
    assert ab.lib().adl_synth_keys16_device(out.ptr, 0x5EED, 3, n, ab._stream()) == 0
    sync(dev)
    assert np.array_equal(out.numpy().reshape(n, 16), oracle.splitmix_keys16(0x5EED, n, skip=3))
    out.check()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_synth_varlen_lengths_output(dev, ab, oracle, n):
    out = Guarded(4 * n, 4, name="d_lengths")
    assert ab.lib().adl_synth_varlen_lengths_device(out.ptr, 0x5EED, n, 1.1, ab._stream()) == 0
    sync(dev)
    want = np.empty(n, np.uint32)
    oracle.lib().oracle_synth_varlen_lengths(0x5EED, n, 1.1, want.ctypes.data)
    assert np.array_equal(out.numpy().view(np.uint32), want)
    out.check()


@pytest.mark.parametrize("total", [1, 7, 8, 9, 4097])
def test_synth_varlen_fill_output(dev, ab, oracle, total):
    """The caller allocates round_up(total_bytes, 8); whole SplitMix words are written."""
    room = (total + 7) // 8 * 8
    out = Guarded(room, 8, name="d_out")
    assert ab.lib().adl_synth_varlen_fill_device(out.ptr, 0x5EED, total, ab._stream()) == 0
    sync(dev)
    want = np.empty(room, np.uint8)
    oracle.lib().oracle_synth_varlen_fill(0x5EED, room, want.ctypes.data)
    assert np.array_equal(out.numpy()[:total], want[:total])
    out.check()


@pytest.mark.parametrize("member", [True, False], ids=["member", "member-null"])
@pytest.mark.parametrize("n,skew", [(1, 0), (255, 1), (256, 3), (257, 0), (1000, 3)])
def test_synth_probe_queries_outputs(dev, ab, oracle, n, skew, member):
    dk = Guarded(16 * n, 16, name="d_keys")
    dfid = Guarded(4 * n, 4, name="d_filter_id")
    dm = Guarded(n, 8, skew=skew, name="d_member")
    rc = ab.lib().adl_synth_probe_queries_device(dk.ptr, dfid.ptr, dm.ptr if member else None, 0xFEED, 12345, n, 7,
                                                 0x5EED, 1000, ab._stream())
    assert rc == 0, rc
    sync(dev)
    k, f, m = oracle.synth_probe_queries(n, seed=0xFEED, q0=12345, num_tables=7, table_seed0=0x5EED,
                                         keys_per_table=1000)
    assert np.array_equal(dk.numpy().reshape(n, 16), k)
    assert np.array_equal(dfid.numpy().view(np.uint32), f)
    if member:
        assert np.array_equal(dm.numpy(), m)
    else:
        assert bool((dm.view == 0xA5).all())  # not written at all
    check_all(dk, dfid, dm)
