"""Host-side inputs for tests/test_gpu_probe_batch_keys.py: filters built by the
oracle from variable-length (or fixed-stride) member keys, and query batches
over them -- half the queries members of their filter, ids drawn from
[0, F + 2), any length per query.  Everything is numpy; nothing here needs a
GPU.
"""
import numpy as np

RUN = 512  # queries per run of hash_run_pairs_kernel (csrc/hash_pairs.hip)


def ragged(starts, lens):
    """Concatenation of the ranges [starts[i], starts[i] + lens[i])."""
    lens = np.asarray(lens, dtype=np.int64)
    before = np.cumsum(lens) - lens
    return np.repeat(np.asarray(starts, dtype=np.int64) - before, lens) + np.arange(int(lens.sum()), dtype=np.int64)


def offsets_of(lens, first=0):
    off = np.empty(len(lens) + 1, dtype=np.uint64)
    off[0] = first
    off[1:] = first + np.cumsum(np.asarray(lens, dtype=np.uint64), dtype=np.uint64)
    return off


def zipf_lengths(oracle, n, seed):
    """n lengths of BASELINE configs[2]'s shape (Zipf, 8-256 B)."""
    _, off = oracle.synth_varlen(n, seed=seed)
    return np.diff(off).astype(np.int64)


class Filters:
    """sizes[t] member keys per filter (None: a range of 0 bytes; 0: the 7-byte
    bitmap of no keys).  Members are oracle.synth_varlen keys, or random keys
    of `stride` bytes.  arena / off: the bitmaps packed back to back."""

    def __init__(self, oracle, sizes, bpk=10, seed=0x5EED, stride=None):
        self.sizes, self.bpk, self.F = list(sizes), bpk, len(sizes)
        counts = np.array([s or 0 for s in sizes], dtype=np.int64)
        total = int(counts.sum())
        if stride is None:
            self.data, self.moff = oracle.synth_varlen(total, seed=seed)
        else:
            rng = np.random.default_rng(seed)
            self.data = rng.integers(0, 256, total * stride + 16, dtype=np.uint8)
            self.moff = offsets_of(np.full(total, stride))
        self.first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)  # filter t's members: first[t]..first[t+1]
        self.counts = counts
        self.bms = []
        for t, s in enumerate(sizes):
            if s is None:
                self.bms.append(np.zeros(0, np.uint8))
            else:
                o = self.moff[self.first[t]:self.first[t + 1] + 1]
                self.bms.append(oracle.keys2block(self.data, o, bits_per_key=bpk))
        self.off = np.concatenate([[0], np.cumsum([b.size for b in self.bms])]).astype(np.uint64)
        self.arena = np.concatenate(self.bms + [np.zeros(16, np.uint8)])

    def scattered(self, seed=1):
        """(arena, begin, end): the same bitmaps in another order with gaps of odd sizes."""
        rng = np.random.default_rng(seed)
        order = rng.permutation(self.F)
        begin, end, o = np.zeros(self.F, np.uint64), np.zeros(self.F, np.uint64), 1001
        for t in order:
            begin[t], end[t] = o, o + self.bms[t].size
            o += self.bms[t].size + int(rng.integers(0, 700))
        arena = np.full(o + 64, 0xFF, np.uint8)
        for t in range(self.F):
            arena[int(begin[t]):int(end[t])] = self.bms[t]
        return arena, begin, end


def queries(filters, n, lens, seed, fixed=None, member_share=0.5):
    """(data, lens, fid, member): n queries with ids from [0, F + 2).  About
    member_share of the queries of a filter that has members are copies of one
    of them (and take its length); every other query has lens[i] random bytes.
    fixed: a bool mask of queries that keep lens[i] whatever else."""
    rng = np.random.default_rng(seed)
    F = filters.F
    fid = rng.integers(0, F + 2, n).astype(np.uint32)
    lens = np.array(lens, dtype=np.int64)
    cnt = np.concatenate([filters.counts, [0, 0]])[fid]
    member = (rng.random(n) < member_share) & (cnt > 0)
    if fixed is not None:
        member &= ~fixed
    sel = np.nonzero(member)[0]
    pick = np.concatenate([filters.first[:-1], [0, 0]])[fid[sel]] + np.minimum((rng.random(sel.size) * cnt[sel]).astype(np.int64),
                                                                                 cnt[sel] - 1)
    mlen = np.diff(filters.moff).astype(np.int64)
    lens[sel] = mlen[pick]
    off = offsets_of(lens)
    total = int(off[-1])
    data = rng.integers(0, 256, total + 16, dtype=np.uint8)
    data[total:] = 0
    if sel.size:
        data[ragged(off[sel].astype(np.int64), lens[sel])] = filters.data[ragged(filters.moff[pick].astype(np.int64),
                                                                                lens[sel])]
    return data, lens, fid, member


def length_sort_changes_every_run(want, lens):
    """True iff moving every answer to its key's place in the run's stable
    sort by min(length, 511) -- the order hash_run_pairs_kernel hashes a run in --
    changes the answers of every run of RUN queries."""
    n = len(want)
    run = np.arange(n) // RUN
    perm = np.argsort(run * 1024 + np.minimum(lens, 511), kind="stable")
    moved = want[perm] != want
    per_run = np.add.reduceat(moved.astype(np.int64), np.arange(0, n, RUN))
    return bool((per_run > 0).all())
