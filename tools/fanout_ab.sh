#!/bin/bash
# tools/fanout_ab.sh -- the level multi-get's two probe paths, interleaved
# (fan-out probe):
#   1. readpath_test --bench (16 tables, about 3.2 candidates per key; 1 000
#      and 65 536 keys) with the default path selection and with the pair path
#      (ADL_BLOOM_LEVEL_FANOUT=0), and -- when PARENT_BIN names a readpath_test
#      built from another commit -- that one first;
#   2. level_fanout_test --bench at 1, 1.3, 1.9 and 3.4 candidates per key,
#      fan-out forced (2) against the pair path (0): where the crossover lies.
# Three repetitions each, one JSON line per run in $OUT/fanout_ab.jsonl.  Every
# GPU step has its own time limit and a failing one ends the script.
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out_fanout}
BIN=adlsm-tree_amd/bin
mkdir -p "$OUT"
: > "$OUT/fanout_ab.jsonl"

run() {  # run <label> <switch or -> <cmd...>
  local label=$1 sw=$2 line; shift 2
  if [ "$sw" = - ]; then line=$(timeout -k 10 120 "$@" | tail -n 1)
  else line=$(ADL_BLOOM_LEVEL_FANOUT=$sw timeout -k 10 120 "$@" | tail -n 1); fi
  [ -n "$line" ] || { echo "FAILED: $label $*"; exit 1; }
  echo "{\"run\": \"$label\", \"rep\": $rep, \"result\": $line}" | tee -a "$OUT/fanout_ab.jsonl"
}

for rep in 1 2 3; do
  [ -n "${PARENT_BIN:-}" ] && run parent - "$PARENT_BIN" --bench
  run default - $BIN/readpath_test --bench
  run pairs 0 $BIN/readpath_test --bench
done
for rep in 1 2 3; do
  for geo in "200000 200000" "150000 200000" "100000 200000" "50000 200000"; do
    for keys in 1000 65536; do
      run fanout 2 $BIN/level_fanout_test --bench 16 $geo $keys
      run pairs 0 $BIN/level_fanout_test --bench 16 $geo $keys
    done
  done
done
exit 0
