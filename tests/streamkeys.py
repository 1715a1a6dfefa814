"""Shared inputs of the streamed-build tests (tests/test_gpu_stream_build.py,
tests/test_stream_build_cpu.py): key sets in the three key shapes, batch
slicing for host and device appends, and oracle bitmaps computed once per
(key set, bounds, bits_per_key) and never modified.

A key set is (data, offs): data (n, stride) uint8 with offs None, or packed
bytes with offs uint64[n + 1].
"""
import numpy as np

N_SPLIT = 6145  # test 1's sequence: more than one pass-A chunk at bpk 10, no multiple of a run

_cache = {}


def keyset(shape, n, seed=1):
    """shape: "k16" 16-byte SplitMix64 keys, "var" keys of 0-69 random bytes
    (every byte value, so bytes >= 0x80 too), "s24" a 24-byte stride."""
    key = ("keys", shape, n, seed)
    if key not in _cache:
        import oracle as O

        rng = np.random.default_rng(seed)
        if shape == "k16":
            ks = (O.splitmix_keys16(0xABC0 + seed, n), None)
        elif shape == "s24":
            ks = (rng.integers(0, 256, size=(n, 24), dtype=np.uint8), None)
        elif shape == "var":
            ks = from_lengths(rng.integers(0, 70, size=n), rng)
        else:
            raise KeyError(shape)
        for a in ks:
            if a is not None:
                a.setflags(write=False)
        _cache[key] = ks
    return _cache[key]


def from_lengths(lengths, rng):
    """Variable-length keys of the given lengths, random bytes 0..255."""
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    data = rng.integers(0, 256, size=max(int(offs[-1]), 1), dtype=np.uint8)
    return data, offs


def from_list(keys):
    """list[bytes] -> a var-len key set."""
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(k) for k in keys], dtype=np.uint64)
    data = np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8).copy()
    return data, offs


def count(ks):
    data, offs = ks
    return data.shape[0] if offs is None else len(offs) - 1


def part(ks, a, b):
    """Keys [a, b) as a key set of their own (offsets from 0)."""
    data, offs = ks
    if offs is None:
        return np.ascontiguousarray(data[a:b]), None
    o = np.ascontiguousarray(offs[a:b + 1] - offs[a])
    d = np.ascontiguousarray(data[int(offs[a]):int(offs[b])])
    return (d if d.size else np.zeros(1, np.uint8)), o  # (a batch of empty keys still has a buffer)


def part_absolute(ks, a, b):
    """Keys [a, b) for a host append the way a caller with one big buffer passes
    them: the whole buffer and the batch's own slice of the offsets (not from 0)."""
    data, offs = ks
    if offs is None:
        return np.ascontiguousarray(data[a:b]), None
    return data, np.ascontiguousarray(offs[a:b + 1])


def to_device(batch, skew=None, keep=None):
    """A batch as device tensors.  skew None: a fresh (256-byte aligned) tensor;
    otherwise the key bytes sit `skew` bytes past a 16-byte boundary that is no
    32-byte boundary, between 0xFF bytes (guardband.Poisoned)."""
    import torch

    data, offs = batch
    doffs = None if offs is None else torch.from_numpy(offs.copy()).cuda()
    if skew is None:
        d = torch.from_numpy(np.ascontiguousarray(data).copy()).cuda()
        return d, doffs
    from guardband import Poisoned

    p = Poisoned(data, 16, skew=skew)
    if keep is not None:
        keep.append(p)
    flat = p.buf[p.start:p.start + p.nbytes]
    assert p.nbytes == 0 or flat.data_ptr() % 16 == skew % 16
    return (flat if offs is not None else flat.reshape(data.shape)), doffs


def oracle_bitmaps(ks, kb, bpk, tag):
    """Keys2Block of every filter [kb[f], kb[f+1]) (cached under `tag`)."""
    key = ("bm", tag, tuple(int(x) for x in kb), bpk)
    if key not in _cache:
        import oracle as O

        out = []
        for f in range(len(kb) - 1):
            d, o = part(ks, int(kb[f]), int(kb[f + 1]))
            if o is None:
                bm = O.keys2block(d.reshape(-1, ks[0].shape[1]), bits_per_key=bpk)
            else:
                bm = O.keys2block(d, offsets=o, bits_per_key=bpk)
            bm = np.array(bm, dtype=np.uint8)
            bm.setflags(write=False)
            out.append(bm)
        _cache[key] = out
    return _cache[key]


def finished(sb, bpk, flags=0, stream=None):
    """finish() downloaded: list of per-filter bitmaps (exact sizes)."""
    import torch

    out, boff, sizes = sb.finish(bpk, flags=flags, stream=stream)
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    h = out.cpu().numpy()
    return [h[int(o):int(o) + int(s)] for o, s in zip(boff, sizes)]


def assert_bitmaps(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size, (what, f, g.size, w.size)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: filter {f}: {bad.size} of {g.size} bytes differ, the first at {bad[0]}"
