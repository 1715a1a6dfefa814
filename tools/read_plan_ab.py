#!/usr/bin/env python3
"""The read plan made in one call against what came before it (DESIGN.md §5,
"Read plan"): adlsm-tree_amd/bin/read_plan_test --bench over the shapes of the
measurement, three rounds with the shapes interleaved.  Each process times, with
their repetitions alternating, RevisionMultiGetFilter followed by
GroupHitsByTable on the host (the parent's path to a plan) and one
RevisionReadPlanFilter call (the grouping on the device), both forced onto the
device call.  Needs a GPU.

  python tools/read_plan_ab.py [OUTDIR]

Shapes: five levels of 16 tables (80 tables: the sort is one pass), and the same
with the bottom level cut into 2 000 tables (2 064: two passes); 1 000, 3 000,
16 000 and 65 536 keys, all absent and all present.  Beside them the device time of
the grouping kernels alone (adl_bloom_hits_by_table_device between two events,
on hit arrays of the same key, hit and table counts).

Every JSON line goes to OUTDIR/read_plan_ab.jsonl, the kernel times to
OUTDIR/kernels.jsonl and the table -- per shape the median of the rounds'
medians with their min-max, which is the run-to-run spread a difference has to
exceed -- to OUTDIR/summary.txt.  OUTDIR defaults to profiles/read_plan."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "adlsm-tree_amd", "bin", "read_plan_test")
ROUNDS = 3
SHAPES = [(5, 16, 0), (5, 16, 2000)]  # (levels, tables per level, tables of the bottom level when it is cut)
KEYS = "1000,3000,16000,65536"


def kernel_ms(keys, hits, num_tables, reps=50):
    """Median device time of one adl_bloom_hits_by_table_device call on `hits` hits of `keys` keys spread evenly
    over the keys and, without a repeat inside a key's list, over the tables."""
    sys.path.insert(0, os.path.join(ROOT, "adlsm-tree_amd"))
    import torch

    import adlbloom as ab

    rng = np.random.default_rng(keys + hits)
    cnt = np.full(keys, hits // keys, np.int64)
    cnt[rng.permutation(keys)[:hits % keys]] += 1
    hb = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    owner = np.repeat(np.arange(keys), cnt)
    j = np.arange(hits) - hb.astype(np.int64)[owner]
    step = np.maximum(1, num_tables // np.maximum(cnt, 1))
    ht = ((rng.integers(0, num_tables, keys)[owner] + j * step[owner]) % num_tables).astype(np.uint32)
    d_hb = torch.from_numpy(hb.view(np.int32)).cuda()
    d_ht = torch.from_numpy(np.concatenate([ht, np.zeros(1, np.uint32)]).view(np.int32)).cuda()
    gcap = min(num_tables, max(hits, 1))
    wsb = ab.lib().adl_bloom_hits_by_table_workspace_bytes(keys, hits, num_tables)
    gt = torch.empty(gcap, dtype=torch.int32, device="cuda")
    gb = torch.empty(gcap + 1, dtype=torch.int32, device="cuda")
    ek = torch.empty(max(hits, 1), dtype=torch.int32, device="cuda")
    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    ws = ab.empty_device(wsb)
    stream = torch.cuda.current_stream()
    ms = []
    for i in range(reps + 5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        rc = ab.lib().adl_bloom_hits_by_table_device(d_hb.data_ptr(), d_ht.data_ptr(), keys, num_tables, gt.data_ptr(),
                                                     gb.data_ptr(), gcap, ek.data_ptr(), hits, counts.data_ptr(),
                                                     ws.data_ptr(), wsb, ctypes.c_void_p(stream.cuda_stream))
        t1.record(stream)
        t1.synchronize()
        if rc != 0:
            raise RuntimeError(f"adl_bloom_hits_by_table_device: status {rc}")
        if i >= 5:
            ms.append(t0.elapsed_time(t1))
    assert int(counts[0].item()) == hits
    return statistics.median(ms), min(ms), max(ms), int(counts[1].item())


def main(argv):
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "read_plan")
    os.makedirs(out, exist_ok=True)
    rows = []
    with open(os.path.join(out, "read_plan_ab.jsonl"), "w") as log:
        for rnd in range(ROUNDS):
            for L, T, bottom in SHAPES:
                r = subprocess.run([EXE, "--bench", str(L), str(T), KEYS, str(bottom)], capture_output=True, text=True,
                                   timeout=240)
                if r.returncode != 0:
                    print("FAILED", L, T, bottom, r.returncode, r.stdout[-500:], r.stderr[-2000:])
                    return 1  # nothing more on the GPU after a failure
                for line in r.stdout.splitlines():
                    d = json.loads(line)
                    d["round"] = rnd
                    rows.append(d)
                    log.write(json.dumps(d) + "\n")
                    log.flush()
    groups = {}
    for d in rows:
        groups.setdefault((d["levels"], d["bottom_tables"], d["keys"], d["batch"]), []).append(d)
    lines = []
    with open(os.path.join(out, "kernels.jsonl"), "w") as klog:
        for (L, bottom, nkeys, batch), ds in groups.items():
            def col(name):
                v = [d[name] for d in ds]
                return "%.4f (%.4f-%.4f)" % (statistics.median(v), min(v), max(v))
            d = ds[0]
            med, lo, hi, groups_seen = kernel_ms(nkeys, d["hits"], d["num_tables"])
            klog.write(json.dumps({"keys": nkeys, "hits": d["hits"], "num_tables": d["num_tables"], "groups": groups_seen,
                                   "grouping_kernels_ms": med, "min": lo, "max": hi}) + "\n")
            shape = "%d x readpath 16" % L + (" (bottom %d)" % bottom if bottom else "")
            lines.append("%28s %6d keys %8s %8d hits %5d groups | multi-get + host grouping %s, the grouping %s | "
                         "read plan %s | grouping kernels alone %.4f (%.4f-%.4f)" % (
                             shape, nkeys, batch, d["hits"], d["groups"], col("multiget_then_host_ms"),
                             col("host_grouping_ms"), col("read_plan_ms"), med, lo, hi))
    with open(os.path.join(out, "summary.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
