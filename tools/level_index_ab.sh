#!/bin/bash
# tools/level_index_ab.sh -- the level multi-get over a resident LevelIndex
# against the per-call selection, interleaved (resident level
# index):
#   * level_index_test --bench-readpath (readpath_test --bench's level: 16
#     tables, about 3.2 candidates per key) at 1 000 and 65 536 keys (or the
#     batch sizes in $KEYS: the crossover between the two index paths);
#   * level_index_test --bench at 1, 1.3, 1.9 and 3.4 candidates per key
#     (level_fanout_test --bench's levels) and on a 2 000-table disjoint level;
#   each with ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS=0 (the host copy of the index)
#   and =1 (selection on the device).  Every run also times
#   LevelMultiGetFilter(cache, tables, ...) and LevelCandidates alone in the
#   same process;
#   * this tree's level_fanout_test --bench (the per-call selection alone in
#     its process), and
#   * when PARENT_BIN names a directory with readpath_test and
#     level_fanout_test built from another commit: those on the same levels.
# Three repetitions, one JSON line per run in $OUT/level_index_ab.jsonl.  Every
# GPU step has its own time limit and a failing one ends the script.
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out_level_index}
BIN=adlsm-tree_amd/bin
KEYS=${KEYS:-1000 65536}
mkdir -p "$OUT"
: > "$OUT/level_index_ab.jsonl"

run() {  # run <label> <min keys or -> <cmd...>
  local label=$1 sw=$2 line; shift 2
  if [ "$sw" = - ]; then line=$(timeout -k 10 120 "$@" | tail -n 1)
  else line=$(ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS=$sw timeout -k 10 120 "$@" | tail -n 1); fi
  [ -n "$line" ] || { echo "FAILED: $label $*"; exit 1; }
  echo "{\"run\": \"$label\", \"rep\": $rep, \"result\": $line}" | tee -a "$OUT/level_index_ab.jsonl"
}

GEOS=("16 200000 200000" "16 150000 200000" "16 100000 200000" "16 50000 200000" "2000 1000 1000")
for rep in 1 2 3; do
  [ -n "${PARENT_BIN:-}" ] && run parent_readpath - "$PARENT_BIN/readpath_test" --bench
  for keys in $KEYS; do
    run readpath_index_host 0 $BIN/level_index_test --bench-readpath $keys
    run readpath_index_device 1 $BIN/level_index_test --bench-readpath $keys
  done
  for geo in "${GEOS[@]}"; do
    for keys in $KEYS; do
      [ -n "${PARENT_BIN:-}" ] && run parent_fanout - "$PARENT_BIN/level_fanout_test" --bench $geo $keys
      run tree_fanout - $BIN/level_fanout_test --bench $geo $keys
      run index_host 0 $BIN/level_index_test --bench $geo $keys
      run index_device 1 $BIN/level_index_test --bench $geo $keys
    done
  done
done
exit 0
