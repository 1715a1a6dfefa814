#!/usr/bin/env python3
"""A/B of the write-through filter cache: what one flush costs until its table's
filter is both in the file buffer and resident in the cache.

For one table of 16-byte keys (bits_per_key 10, pinned host buffers) three
variants are timed per flush, interleaved repetition by repetition on one
device in one process:

  (a) parent   adl_bloom_build_segmented into the host block, the trailer framed
               on the host, then adl_bloom_filter_cache_put (the re-upload)
  (b) build    adl_bloom_filter_cache_build + adl_bloom_filter_cache_publish
  (c) verify   (b) with ADL_BLOOM_CACHE_VERIFY

The baseline is (a) of the same run.  Every repetition's three blocks are
compared byte for byte.  One JSON line per repetition and one summary line per
key count (medians, min, max) go to --out; the summary table is printed.

  python tools/write_through_ab.py [--ns 1000000,10000000] [--reps 9] [--out profiles/write_through/ab.jsonl]
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adlsm-tree_amd"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_through", "ab.jsonl"))
    args = ap.parse_args()

    import torch

    import adlbloom as ab

    L = ab.lib()
    bpk = 10
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []
    for n in [int(x) for x in args.ns.split(",")]:
        keys = torch.empty((n, 16), dtype=torch.uint8, pin_memory=True)
        keys.copy_(ab.synth_keys16(n, seed=0x5EED))
        torch.cuda.synchronize()
        kb = np.array([0, n], dtype=np.uint64)
        off0 = np.zeros(1, dtype=np.uint64)
        nbytes = ab.filter_block_bytes(kb, bpk)
        region = ab.bitmap_bytes(n, bpk)
        blocks = {v: torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True) for v in "abc"}
        trailer = np.frombuffer(struct.pack("<iii", 0, region, 1) + b"bf:" + struct.pack("<ii", bpk, 7), dtype=np.uint8)
        cache = ab.FilterCache(2 * nbytes + (1 << 20), max_tables=4)
        oid = b"flush"

        def parent():
            b = blocks["a"]
            ab._check(L.adl_bloom_build_segmented(keys.data_ptr(), None, 16, kb.ctypes.data, 1, bpk, b.data_ptr(),
                                                  off0.ctypes.data, None), "build_segmented")
            b.numpy()[region:] = trailer
            ab._check(L.adl_bloom_filter_cache_put(cache._h, oid, len(oid), b.data_ptr(), nbytes), "put")

        def through(which, flags):
            b = blocks[which]
            t = ctypes.c_void_p()
            ab._check(L.adl_bloom_filter_cache_build(cache._h, keys.data_ptr(), None, 16, kb.ctypes.data, 1, bpk,
                                                     flags, b.data_ptr(), nbytes, ctypes.byref(t), None), "build")
            ab._check(L.adl_bloom_filter_cache_publish(cache._h, t, oid, len(oid)), "publish")

        variants = [("a", parent), ("b", lambda: through("b", 0)), ("c", lambda: through("c", ab.CACHE_VERIFY))]
        times = {v: [] for v, _ in variants}
        for rep in range(args.warmup + args.reps):
            row = {}
            for v, fn in variants:
                t0 = time.perf_counter()
                fn()
                row[v] = (time.perf_counter() - t0) * 1e3
                assert oid in cache
                cache.remove(oid)  # (outside the timing: every flush starts with an empty arena)
            same = all(bytes(blocks[v].numpy()) == bytes(blocks["a"].numpy()) for v in "bc")
            assert same, "the variants' blocks differ"
            if rep >= args.warmup:
                for v in row:
                    times[v].append(row[v])
                lines.append({"n": n, "rep": rep - args.warmup, "ms": {k: round(x, 4) for k, x in row.items()},
                              "blocks_equal": same})
        summ = {"n": n, "bits_per_key": bpk, "block_bytes": nbytes, "reps": args.reps, "summary": {}}
        for v in times:
            a = np.array(times[v])
            summ["summary"][v] = {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
                                  "max_ms": round(float(a.max()), 4)}
        med = {v: summ["summary"][v]["median_ms"] for v in times}
        summ["b_over_a"] = round(med["b"] / med["a"], 4)
        summ["c_over_b"] = round(med["c"] / med["b"], 4)
        lines.append(summ)
        print(f"n = {n}: block {nbytes} B")
        for v, name in (("a", "build_segmented + put"), ("b", "cache build + publish"), ("c", "(b) + CACHE_VERIFY")):
            s = summ["summary"][v]
            print(f"  ({v}) {name:24s} median {s['median_ms']:9.3f} ms   min {s['min_ms']:9.3f}   max {s['max_ms']:9.3f}")
        print(f"  (b)/(a) = {summ['b_over_a']:.3f}   (c)/(b) = {summ['c_over_b']:.3f}")
        cache.close()
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
