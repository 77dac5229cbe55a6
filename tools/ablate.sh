#!/bin/bash
# Library-variant sweep: one bench per variant (kernel times via HIP events).
set -u
ROOT="$(cd "$(dirname "$0")/.." && pwd)"; cd "$ROOT"; OUT="${OUT:-bench_out}"; mkdir -p "$OUT"/ablate
for v in ${VARIANTS:-base}; do
  lib="$ROOT/radar-signal-process_amd/lib/librsp.so"; [ $v != base ] && lib="$ROOT/radar-signal-process_amd/lib/ablate/librsp_$v.so"
  for st in ${STREAMS:-1 2}; do
    RSP_LIB=$lib timeout -k 10 200 python bench.py --full --steps 5 --warmup 1 --cpu-seconds 0 --streams $st ${BENCH_ARGS:-} > $OUT/ablate/${v}_s$st.json 2>/dev/null || exit $?
  done
  echo "$v done"
done
