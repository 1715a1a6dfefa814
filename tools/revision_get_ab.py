#!/usr/bin/env python3
"""The single-key revision Get against the one-key revision multi-get (DESIGN.md
§5, "Single-key revision Get"): adlsm-tree_amd/bin/revision_get_test --bench
over 1, 3 and 5 levels of the read-path shape, absent keys and keys present in
every level, 13- and 64-byte keys; three rounds with the shapes interleaved
(each process times both ways in alternating blocks of 100 calls).  Needs a GPU.

  python tools/revision_get_ab.py [OUTDIR] [--parent DIR]

Every JSON line goes to OUTDIR/revision_get_ab.jsonl and the table -- per shape
the median of the rounds' medians with their min-max, the p99 likewise, and how
many of the Gets the resident server answered -- to OUTDIR/summary.txt.
OUTDIR defaults to profiles/revision_get.

--parent DIR: the regression guard of the plain single-key Get as well.  DIR
holds a build of the parent commit (DIR/adlsm-tree_amd/bin/readpath_test);
its `readpath_test --bench` and this tree's run in turn, seven rounds each,
into OUTDIR/single_key_guard.jsonl, the summary appended to summary.txt."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "adlsm-tree_amd", "bin", "revision_get_test")
ROUNDS = 3
GUARD_ROUNDS = 7


def spread(v, fmt="%.2f"):
    return (fmt + " (" + fmt + "-" + fmt + ")") % (statistics.median(v), min(v), max(v))


def guard(parent, out, lines):
    exes = {"parent": os.path.join(parent, "adlsm-tree_amd", "bin", "readpath_test"),
            "this": os.path.join(ROOT, "adlsm-tree_amd", "bin", "readpath_test")}
    rows = {"parent": [], "this": []}
    with open(os.path.join(out, "single_key_guard.jsonl"), "w") as log:
        for rnd in range(GUARD_ROUNDS):
            for who, exe in exes.items():  # interleaved: a drift of the machine meets both alike
                r = subprocess.run([exe, "--bench"], capture_output=True, text=True, timeout=240)
                if r.returncode != 0:
                    print("FAILED", who, r.returncode, r.stdout[-500:], r.stderr[-2000:])
                    return 1  # nothing more on the GPU after a failure
                d = json.loads(r.stdout.splitlines()[-1])
                rows[who].append(d)
                log.write(json.dumps({"build": who, "round": rnd, **d}) + "\n")
                log.flush()
    lines.append("")
    lines.append("plain single-key IsKeyExists, readpath_test --bench, %d interleaved rounds (us)" % GUARD_ROUNDS)
    for who in ("parent", "this"):
        med = [d["single_key_is_key_exists_us"]["median"] for d in rows[who]]
        p99 = [d["single_key_is_key_exists_us"]["p99"] for d in rows[who]]
        lines.append("%8s median %s   p99 %s" % (who, spread(med, "%.1f"), spread(p99, "%.1f")))
    return 0


def main(argv):
    parent = None
    if "--parent" in argv:
        i = argv.index("--parent")
        parent = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "revision_get")
    shapes = [(L, kb, kind) for L in (1, 3, 5) for kb in (13, 64) for kind in ("absent", "present")]
    os.makedirs(out, exist_ok=True)
    rows = []
    with open(os.path.join(out, "revision_get_ab.jsonl"), "w") as log:
        for rnd in range(ROUNDS):
            for L, kb, kind in shapes:
                r = subprocess.run([EXE, "--bench", str(L), "16", str(kb), kind], capture_output=True, text=True,
                                   timeout=240)
                if r.returncode != 0:
                    print("FAILED", L, kb, kind, r.returncode, r.stdout[-500:], r.stderr[-2000:])
                    return 1  # nothing more on the GPU after a failure
                d = json.loads(r.stdout.splitlines()[-1])
                d["round"] = rnd
                rows.append(d)
                log.write(json.dumps(d) + "\n")
                log.flush()
    lines = ["us per call: the median of %d processes' medians (min-max); served = requests the resident server "
             "answered per call" % ROUNDS]
    for L, kb, kind in shapes:
        ds = [d for d in rows if (d["levels"], d["key_bytes"], d["keys"]) == (L, kb, kind)]
        calls = ds[0]["calls"]
        lines.append(
            "%d x readpath 16, %2d-byte %-7s keys, %5.2f candidates | Get %s p99 %s served %.2f | per-level %s p99 %s "
            "served %.2f | launches %d" % (
                L, kb, kind, ds[0]["candidates_per_key"], spread([d["get_us"] for d in ds]),
                spread([d["get_p99_us"] for d in ds]), statistics.mean(d["get_requests_served"] for d in ds) / calls,
                spread([d["per_level_us"] for d in ds]), spread([d["per_level_p99_us"] for d in ds]),
                statistics.mean(d["per_level_requests_served"] for d in ds) / calls,
                max(d["server_launches"] for d in ds)))
    rc = guard(parent, out, lines) if parent else 0
    text = "\n".join(lines) + "\n"
    with open(os.path.join(out, "summary.txt"), "w") as f:
        f.write(text)
    print(text)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
