"""Host-side inputs for the tests of the probes with a probe count per filter
(tests/test_gpu_probe_batch_k.py, tests/test_gpu_cache_probe_batch.py):
filters built by the oracle under different bits_per_key in one arena, and the
oracle's answers for a batch over them.  The oracle takes one bits_per_key per
call, so the answers come from one oracle.probe_multi per distinct bits_per_key,
over the queries bound for that bits_per_key's filters.  Everything is numpy;
nothing here needs a GPU.
"""
import numpy as np

import probekeys as pk


class MixedFilters:
    """spec[t] = (members, bits_per_key) per filter (members None: a range of 0
    bytes; 0: the 7-byte bitmap of no keys).  Members are random keys of
    `stride` bytes, or oracle.synth_varlen keys for stride None.  The
    attributes are those of probekeys.Filters (so probekeys.queries draws
    batches over it), with bpk and k one entry per filter."""

    def __init__(self, oracle, spec, seed, stride=16):
        self.F = len(spec)
        self.bpk = np.array([b for _, b in spec], dtype=np.int64)
        self.k = np.array([oracle.num_probes(int(b)) for b in self.bpk], dtype=np.uint8)
        counts = np.array([s or 0 for s, _ in spec], dtype=np.int64)
        total = int(counts.sum())
        if stride is None:
            self.data, self.moff = oracle.synth_varlen(total, seed=seed)
        else:
            rng = np.random.default_rng(seed)
            self.data = rng.integers(0, 256, total * stride + 16, dtype=np.uint8)
            self.moff = pk.offsets_of(np.full(total, stride))
        self.first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.counts = counts
        self.bms = []
        for t, (s, b) in enumerate(spec):
            if s is None:
                self.bms.append(np.zeros(0, np.uint8))
            else:
                o = self.moff[self.first[t]:self.first[t + 1] + 1]
                self.bms.append(oracle.keys2block(self.data, o, bits_per_key=int(b)))
        self.off = np.concatenate([[0], np.cumsum([b.size for b in self.bms])]).astype(np.uint64)
        self.arena = np.concatenate(self.bms + [np.zeros(16, np.uint8)])

    def scattered(self, seed=1):
        """(arena, begin, end): the same bitmaps in shuffled arena order with gaps."""
        return pk.Filters.scattered(self, seed)


def oracle_answers(oracle, arena, off, bpk_of, data, key_off, fid, stride=None):
    """BloomFilter::IsKeyExists per query, filter f with bits_per_key bpk_of[f];
    0 for an id past the filters.  key_off: the keys' n + 1 offsets."""
    fid = np.asarray(fid)
    F = len(bpk_of)
    want = np.zeros(len(fid), np.uint8)
    in_range = fid < F
    qb = np.where(in_range, np.asarray(bpk_of)[np.minimum(fid, F - 1)], -1)
    key_off = np.asarray(key_off)
    lens = np.diff(key_off).astype(np.int64)
    for b in np.unique(qb[in_range]):
        sel = np.nonzero(qb == b)[0]
        if stride is not None:
            keys = data[:len(fid) * stride].reshape(len(fid), stride)[sel]
            want[sel] = oracle.probe_multi(keys, fid[sel], arena, off, bits_per_key=int(b))
        else:
            sub = np.concatenate([data[pk.ragged(key_off[sel].astype(np.int64), lens[sel])], np.zeros(16, np.uint8)])
            want[sel] = oracle.probe_multi(sub, fid[sel], arena, off, offsets=pk.offsets_of(lens[sel]),
                                           bits_per_key=int(b))
    return want


class MixedBatch:
    """n queries over `flt` (half the queries bound for a filter with members
    are members of it; ids from [0, F + 2)) and the oracle's answers, computed
    once and read-only."""

    def __init__(self, oracle, flt, n, seed, stride=16, lens=None):
        self.flt, self.n, self.stride = flt, n, stride
        lens = np.full(n, stride) if stride is not None else lens
        self.data, self.lens, self.fid, self.member = pk.queries(flt, n, lens, seed)
        self.off = pk.offsets_of(self.lens)
        self.total = int(self.off[-1])
        self.want = oracle_answers(oracle, flt.arena, flt.off, flt.bpk, self.data, self.off, self.fid, stride)
        has_members = np.concatenate([flt.counts, [0, 0]])[self.fid] > 0
        assert self.want[self.member].all() and self.member.sum() > 0.45 * has_members.sum() and not self.want.all()
        assert not self.want[self.fid >= flt.F].any()
        for a in (self.data, self.fid, self.off, self.want):
            a.flags.writeable = False

    @property
    def keys(self):
        """(n, stride) for fixed-stride batches."""
        return self.data[:self.total].reshape(self.n, self.stride)
