#!/usr/bin/env python3
"""tools/level_index_summary.py FILE -- the medians of tools/level_index_ab.sh's
repetitions (level_index_ab.jsonl), one line per level and batch size: the
median of the repetitions' medians with their min and max, in ms.

parent / tree: level_fanout_test --bench (readpath_test --bench for the first
level) of the other commit / of this tree: LevelMultiGetFilter(cache, tables);
host / device: LevelMultiGetFilter(cache, index) with
ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS=0 / =1; sel: LevelCandidates alone.

Lines with a "search" field (search_ab.jsonl: level_index_test --bench with
ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS=0 from two builds of the mirror, with
kBranchFreeMinKeys set so that every batch / no batch searches branch-free)
give one line per level and batch size with the two searches side by side."""
import json
import statistics
import sys
from collections import defaultdict


def main(path):
    rows = defaultdict(lambda: defaultdict(list))
    for line in open(path):
        d = json.loads(line)
        if "search" in d:
            r = d["result"]
            level = "readpath 16" if d["mode"] == "--bench-readpath" else f"{r['tables']} x {r['span']}/{r['stride']}"
            rows[(level, r["keys"])]["branch-free" if d["search"] == "bf" else "branching"].append(r["index_ms"])
            rows[(level, r["keys"])]["pairs"].append(r["pairs_probed"])
            continue
        r, run = d["result"], d["run"]
        if run == "parent_readpath":
            for k in (1000, 65536):
                rows[("readpath 16", k)]["parent"].append(r[f"multiget_{k}_keys"]["median_ms"])
            continue
        level = f"{r['tables']} x {r['span']}/{r['stride']}"
        if run.startswith("readpath_"):  # the script labels --bench-readpath's runs
            level, run = "readpath 16", run[len("readpath_"):]
        key = (level, r["keys"])
        if run in ("parent_fanout", "tree_fanout"):
            rows[key][run[:-7]].append(r["median_ms"])
        else:
            rows[key][run[6:]].append(r["index_ms"])
            rows[key]["sel"].append(r["level_candidates_ms"])
            rows[key]["pairs"].append(r["pairs_probed"])
    for key, v in rows.items():
        cells = []
        for name in ("parent", "tree", "host", "device", "sel", "branching", "branch-free"):
            if name in v:
                x = v[name]
                cells.append(f"{name} {statistics.median(x):.4f} ({min(x):.4f}-{max(x):.4f})")
        pairs = v["pairs"][0] if "pairs" in v else "-"
        print(f"{key[0]:>22} {key[1]:>6} keys {pairs:>7} pairs | " + " | ".join(cells))


if __name__ == "__main__":
    main(sys.argv[1])
