#!/usr/bin/env python3
"""The revision multi-get against one level multi-get per level (DESIGN.md §5,
"Revision multi-get"): adlsm-tree_amd/bin/revision_test --bench over the shapes
of the measurement, three rounds with the shapes interleaved (each process times
both ways with their repetitions alternating).  Needs a GPU.

  python tools/revision_ab.py [--crossover] [OUTDIR]

Every JSON line goes to OUTDIR/revision_ab.jsonl and the table -- per shape the
median of the rounds' medians with their min-max -- to OUTDIR/summary.txt
(--crossover: crossover_ab.jsonl and crossover_summary.txt; 1, 2, 3 and 5 levels
at 250 to 16 000 keys, which is where the overload's thresholds come from).
OUTDIR defaults to profiles/revision."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "adlsm-tree_amd", "bin", "revision_test")
ROUNDS = 3


def main(argv):
    crossover = "--crossover" in argv
    rest = [a for a in argv if a != "--crossover"]
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "revision")
    # (levels, tables per level, tables of the bottom level when it is cut into disjoint ones)
    shapes = [(1, 16, 0), (2, 16, 0), (3, 16, 0), (5, 16, 0)] if crossover else \
        [(1, 16, 0), (3, 16, 0), (5, 16, 0), (5, 16, 2000)]
    keys = "250,500,1000,2000,4000,8000,16000" if crossover else "1000,3000,65536"
    raw, table = ("crossover_ab.jsonl", "crossover_summary.txt") if crossover else ("revision_ab.jsonl", "summary.txt")
    os.makedirs(out, exist_ok=True)
    rows = []
    with open(os.path.join(out, raw), "w") as log:
        for rnd in range(ROUNDS):
            for L, T, bottom in shapes:
                r = subprocess.run([EXE, "--bench", str(L), str(T), keys, str(bottom)], capture_output=True, text=True,
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
    for (L, bottom, nkeys, batch), ds in groups.items():
        def col(name):
            v = [d[name] for d in ds]
            return "%.4f (%.4f-%.4f)" % (statistics.median(v), min(v), max(v))
        d = ds[0]
        shape = "%d x readpath 16" % L + (" (bottom %d)" % bottom if bottom else "")
        lines.append("%28s %6d keys %8s %8d pairs %8d hits | per-level %s | revision %s | d2h %d -> %d B" % (
            shape, nkeys, batch, d["pairs"], d["hits"], col("per_level_ms"), col("revision_ms"), d["d2h_per_level"],
            d["d2h_revision"]))
    with open(os.path.join(out, table), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
