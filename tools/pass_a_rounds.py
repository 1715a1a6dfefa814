#!/usr/bin/env python3
"""tools/pass_a_rounds.py -- pass A's rounds, one by one, on two builds.

Needs the diagnostics library (make -C adlsm-tree_amd stamps, or
ADL_BLOOM_LIB=<a library built with -DADL_BLOOM_STAMPS>): wave 0 of every
pass-A workgroup stores s_memrealtime (100 MHz) at kernel entry, at the top of each
chunk step, at the end of the loop and once the last chunk's stores have left
its counters (ROUND_STAMP in csrc/bloom_build.hip).

  headline   one filter of N keys (default 10 M x 16 B, bpk 10): 7 rounds
  long       FILTERS (default 26) filters of N keys in one launch pair: the
             same T and C, about 180 rounds per workgroup

For each build and each of REPS repetitions it prints one JSON line:
  rounds              chunk steps per workgroup (min, max)
  first_us            kernel entry -> top of step 0 (the first load, exposed,
                      with chunk 0's hashes), median over workgroups
  steady_us           median over workgroups and over steps 1 .. last-1 of a
                      step's duration; steady_by_round_us the median per step
                      (up to 12 steps)
  drain_us            end of the loop -> last stores done, median
  span_us             first entry -> last done over all workgroups
  skew_us             standard deviation over workgroups of the step tops,
                      averaged over the steps: how far the workgroups drift
  pass_a_us           the kernel by HIP events, beside it
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("ADL_BLOOM_LIB", os.path.join(ROOT, "adlsm-tree_amd", "lib_stamps", "libadlbloom.so"))
sys.path.insert(0, os.path.join(ROOT, "adlsm-tree_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import adlbloom as ab  # noqa: E402

TICK_US = 0.01  # s_memrealtime: 100 MHz
NS = 256        # stamps per workgroup (kRoundStamps)


def rounds_of(L):
    buf = np.zeros((256, NS), dtype=np.uint64)
    assert L.adl_bloom_debug_rounds(buf.ctypes.data, buf.size) == 0
    return buf.astype(np.int64)


def summarise(buf, pass_a_ms):
    rows, ids = [], []
    for b, r in enumerate(buf):
        if r[0] == 0:
            continue
        n = 1
        while n < NS and r[n] >= r[n - 1] and r[n] - r[0] < 10**9:  # (stale stamps of an earlier launch end it)
            n += 1
        rows.append(r[:n])  # entry, R step tops, loop end, stores done
        ids.append(b)
    R = [len(r) - 3 for r in rows]
    first = [r[1] - r[0] for r in rows]
    drain = [r[-1] - r[-2] for r in rows]
    steps = [np.diff(np.append(r[1:-2], r[-2])) for r in rows]  # R durations each
    rmin = min(R)
    steady = np.concatenate([s[1:len(s) - 1] for s in steps if len(s) > 2]) if rmin > 2 else np.array([0])
    by_round = [float(np.median([s[i] for s in steps if len(s) > i])) * TICK_US for i in range(min(max(R), 12))]
    # span and skew inside each XCD (workgroups b, b + 8, ...: one clock for certain), then the
    # longest span and the mean skew
    spans, skews = [], []
    for x in range(8):
        grp = [r for b, r in zip(ids, rows) if b % 8 == x]
        if not grp:
            continue
        spans.append(max(r[-1] for r in grp) - min(r[0] for r in grp))
        skews.append(np.array([r[1:1 + rmin] for r in grp]).std(axis=0).mean())
    return {"workgroups": len(rows), "rounds": [int(min(R)), int(max(R))],
            "first_us": round(float(np.median(first)) * TICK_US, 2),
            "steady_us": round(float(np.median(steady)) * TICK_US, 3),
            "steady_mean_us": round(float(np.mean(steady)) * TICK_US, 3),
            "steady_by_round_us": [round(x, 2) for x in by_round],
            "drain_us": round(float(np.median(drain)) * TICK_US, 2),
            "span_us": round(float(max(spans)) * TICK_US, 2),
            "skew_us": round(float(np.mean(skews)) * TICK_US, 3),
            "pass_a_us": round(pass_a_ms * 1e3, 2)}


def main():
    n = int(os.environ.get("N", 10_000_000))
    nf = int(os.environ.get("FILTERS", 26))
    reps = int(os.environ.get("REPS", 5))
    L = ab.lib()
    L.adl_bloom_debug_rounds.restype = ctypes.c_int
    L.adl_bloom_debug_rounds.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    keys = torch.cat([ab.synth_keys16(n, seed=0x5EED + f) for f in range(nf)])
    one = ab.Builder(n, 10)
    seg = ab.SegmentedBuilder(np.arange(nf + 1, dtype=np.uint64) * n, 10)
    builds = {"headline": lambda: one.build(keys[:n]), "long": lambda: seg.build(keys)}
    for name in os.environ.get("BUILDS", "headline,long").split(","):
        for _ in range(2):
            builds[name]()
        torch.cuda.synchronize()
        for rep in range(reps):
            ab.profile_enable(16)
            builds[name]()
            torch.cuda.synchronize()
            ms_a, _, _ = ab.profile_collect()
            print(json.dumps(dict(build=name, rep=rep, lib=os.path.relpath(os.environ["ADL_BLOOM_LIB"], ROOT),
                                  **summarise(rounds_of(L), ms_a))), flush=True)


if __name__ == "__main__":
    main()
