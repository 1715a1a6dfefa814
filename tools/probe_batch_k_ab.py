#!/usr/bin/env python3
"""tools/probe_batch_k_ab.py -- the large-batch probe with a probe count per
filter (adl_bloom_probe_batch_k_device): the tile-binned pipeline against the
direct kernel on the same device inputs, to place the default of
ADL_BLOOM_PROBE_BATCH_MAX_K.

A binned query costs k_f entries whether it is a member or not; the direct
kernel stops at the first clear bit.  So every shape is timed on a batch whose
queries are all members of their filter (the direct kernel reads all k bits)
and on one whose queries are all absent (it reads about two).

Shapes: 256 resident filters of 1 M 16-byte keys; max_k in {2, 6, 7, 11, 30},
uniform (every filter built at the bits_per_key whose k is max_k) and mixed
(tables 0..127 at bits_per_key 10, k = 6, the others at max_k's; max_k >= 7
only: at 6 it is the uniform shape, at 2 a table of k = 6 is past max_k);
n in {2^20, 2^22, 2^24, 10^8}.

Per shape the two paths run in one process on the same tensors, interleaved
rep by rep (one warm-up rep each, then `reps`), the knob set to 30 (binned) and
0 (direct) and re-read between calls; each call is timed with device events
around it and the line gives medians with min-max.  The two answer arrays are
compared byte for byte on the device, and a member batch must answer 1
throughout; the direct kernel itself is held to the oracle by tests/.

usage: python tools/probe_batch_k_ab.py [--reps R] [--out DIR] [--max-k K,K...] [--queries N,N...]
One JSON line per (layout, max_k, n, kind) on stdout; --out also writes
raw.jsonl and summary.md there.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adlsm-tree_amd"))
import adlbloom as ab  # noqa: E402

KNOB = "ADL_BLOOM_PROBE_BATCH_MAX_K"
BPK_OF_K = {2: 3, 6: 10, 7: 11, 11: 16, 30: 44}  # num_probes(bpk) = (int)(bpk * 0.69)
F, PER = 256, 1_000_000


def u64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64)).cuda()


def build(keys, first, count, bpk):
    """`count` filters of PER keys from filter `first` on: (bitmaps, begin, end) with offsets into bitmaps."""
    kb = np.arange(count + 1, dtype=np.uint64) * PER
    bms, boff, nbytes = ab.build_segmented(keys[first * PER:(first + count) * PER], kb, bits_per_key=bpk)
    return bms, np.asarray(boff, np.uint64), np.asarray(boff, np.uint64) + np.asarray(nbytes, np.uint64)


def arena_for(keys, layout, max_k):
    if layout == "uniform":
        bms, begin, end = build(keys, 0, F, BPK_OF_K[max_k])
        k = np.full(F, max_k, np.uint8)
    else:
        a, ab0, ae0 = build(keys, 0, F // 2, 10)
        b, bb0, be0 = build(keys, F // 2, F // 2, BPK_OF_K[max_k])
        pad = (-a.numel()) % 256
        bms = torch.cat([a, torch.zeros(pad, dtype=torch.uint8, device="cuda"), b])
        shift = np.uint64(a.numel() + pad)
        begin, end = np.concatenate([ab0, bb0 + shift]), np.concatenate([ae0, be0 + shift])
        k = np.concatenate([np.full(F // 2, 6, np.uint8), np.full(F // 2, max_k, np.uint8)])
        del a, b
    return bms, u64(begin), u64(end), torch.from_numpy(k).cuda()


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def set_knob(v):
    os.environ[KNOB] = str(v)
    ab.reload_knobs()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-k", default="2,6,7,11,30")
    ap.add_argument("--queries", default=f"{1 << 20},{1 << 22},{1 << 24},{10 ** 8}")
    args = ap.parse_args()
    ks = [int(x) for x in args.max_k.split(",")]
    ns = [int(x) for x in args.queries.split(",")]
    assert all(k in BPK_OF_K and ab.num_probes(BPK_OF_K[k]) == k for k in ks)
    torch.cuda.set_device(0)
    saved = os.environ.get(KNOB)
    keys = ab.synth_keys16(F * PER, seed=0x5EED, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(0xAB)
    nmax = max(ns)
    fid = torch.randint(0, F, (nmax,), device="cuda", generator=g, dtype=torch.int64)
    pick = fid * PER + torch.randint(0, PER, (nmax,), device="cuda", generator=g, dtype=torch.int64)
    batches = {"member": keys[pick], "absent": ab.synth_keys16(nmax, seed=0xFEED, device="cuda")}
    d_fid = fid.to(torch.int32)
    del pick, fid
    lines = []
    for layout, max_k in [("uniform", k) for k in ks] + [("mixed", k) for k in ks if k > 6]:
        bms, begin, end, d_k = arena_for(keys, layout, max_k)
        for n in ns:
            set_knob(30)
            ws = ab.empty_device(ab.lib().adl_bloom_probe_batch_k_workspace_bytes(n, F, max_k, 16))
            for kind, q in batches.items():
                outs = {m: torch.empty(n, dtype=torch.uint8, device="cuda") for m in ("binned", "direct")}
                ts = {m: [] for m in outs}
                for r in range(args.reps + 1):  # rep 0 warms each path up
                    for m, v in (("binned", 30), ("direct", 0)):
                        set_knob(v)
                        t = timed(lambda: ab.probe_batch_k(q[:n], d_fid[:n], bms, begin, d_k, max_k, bitmap_end=end,
                                                           out=outs[m], workspace=ws))
                        if r:
                            ts[m].append(t)
                same = bool(torch.equal(outs["binned"], outs["direct"]))
                ones = float(outs["binned"].float().mean().item())
                assert same, (layout, max_k, n, kind)
                assert kind != "member" or ones == 1.0
                line = {"layout": layout, "max_k": max_k, "filters": F, "keys_per_filter": PER, "queries": n,
                        "batch": kind, "answers_equal": same, "share_answered_1": round(ones, 6)}
                for m in outs:
                    line[f"ms_{m}_median"] = round(float(np.median(ts[m])), 4)
                    line[f"ms_{m}_min"] = round(min(ts[m]), 4)
                    line[f"ms_{m}_max"] = round(max(ts[m]), 4)
                line["binned_over_direct"] = round(line["ms_binned_median"] / line["ms_direct_median"], 4)
                print(json.dumps(line), flush=True)
                lines.append(line)
            del ws
            torch.cuda.empty_cache()
        del bms, begin, end, d_k
        torch.cuda.empty_cache()
    if saved is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = saved
    ab.reload_knobs()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "raw.jsonl"), "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)
        with open(os.path.join(args.out, "summary.md"), "w") as f:
            f.write(f"median ms (min-max) of {args.reps} interleaved reps; 256 filters x 1 M keys, 16-byte queries\n\n")
            f.write("| layout | max_k | queries | batch | binned ms | direct ms | binned / direct |\n|---|---|---|---|---|---|---|\n")
            for x in lines:
                f.write(f"| {x['layout']} | {x['max_k']} | {x['queries']} | {x['batch']} | "
                        f"{x['ms_binned_median']} ({x['ms_binned_min']}-{x['ms_binned_max']}) | "
                        f"{x['ms_direct_median']} ({x['ms_direct_min']}-{x['ms_direct_max']}) | "
                        f"{x['binned_over_direct']} |\n")


if __name__ == "__main__":
    main()
