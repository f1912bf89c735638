#!/bin/bash
# On an MI355X: GPU parity tests, smoke, bench (--full), rocprofv3 kernel-trace summary.  Logs -> $Y5_CHECK_OUT (default check_out/).
cd "$(dirname "$0")/.."
OUT="${Y5_CHECK_OUT:-check_out}"
mkdir -p "$OUT" && OUT="$(cd "$OUT" && pwd)"
export TMPDIR=/tmp
WHAT="${1:-all}"
if [ "$WHAT" = "all" ] || [ "$WHAT" = "test" ]; then
  timeout 900 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?" | tee -a $OUT/pytest_gpu.log
  tail -25 $OUT/pytest_gpu.log
  timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke rc=$?" | tee -a $OUT/smoke.log
  tail -3 $OUT/smoke.log
fi
if [ "$WHAT" = "all" ] || [ "$WHAT" = "bench" ]; then
  timeout 600 python bench.py --full --op-table $OUT/op_table.json > $OUT/bench.log 2>&1; echo "bench rc=$?" | tee -a $OUT/bench.log
  tail -5 $OUT/bench.log
  timeout 300 python scripts/metrics_bench.py > $OUT/metrics_bench.log 2>&1; tail -2 $OUT/metrics_bench.log
  timeout 300 python scripts/letterbox_bench.py > $OUT/letterbox_bench.log 2>&1; tail -2 $OUT/letterbox_bench.log
fi
if [ "$WHAT" = "all" ] || [ "$WHAT" = "prof" ]; then
  rm -rf $OUT/prof
  # tile choices cached by a first run: the profiled run launches no autotune timing kernels
  export Y5_TUNE_CACHE=/tmp/y5_tune_prof.json
  [ -n "$Y5_SEED_TUNE_CACHE" ] && [ -f "$Y5_SEED_TUNE_CACHE" ] && cp "$Y5_SEED_TUNE_CACHE" "$Y5_TUNE_CACHE"   # (scripts/r6_final.sh: the timed run's choices)
  timeout 600 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-train --no-configs --no-selfcheck > /dev/null 2>&1
  (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o r -- python "$OLDPWD/bench.py" --full --steps 10 --warmup 3 --no-cpu-baseline --no-train --no-configs --no-selfcheck > "$OUT/prof.log" 2>&1); echo "prof rc=$?"
  find $OUT/prof -name "*stats*" | head; 
  f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -30 "$f"
  t=$(find $OUT/prof -name "*kernel_trace.csv" | head -1)
  gb=$(python -c "import json,re,sys; l=[x for x in open('$OUT/prof.log') if x.startswith('{')][-1]; print(json.loads(l)['roofline']['algorithmic_gbytes_per_step'])")
  gf=$(python -c "import json,re,sys; l=[x for x in open('$OUT/prof.log') if x.startswith('{')][-1]; print(json.loads(l)['roofline']['algorithmic_gflop_per_step'])")
  [ -n "$t" ] && python scripts/rocprof_frac.py "$t" --gbytes "$gb" --gflop "$gf" --out $OUT/prof/rocprof_frac.json | head -30
  grep '^{' $OUT/prof.log | tail -1 > $OUT/prof/bench_line.json
  # keep the merged-back directory small: drop the raw per-dispatch trace, keep the summaries
  find $OUT/prof -name "*kernel_trace.csv" -size +20M -delete
fi
if [ "$WHAT" = "all" ] || [ "$WHAT" = "train" ]; then
  # training step: per-kernel summary with warm tile / split choices (the first plain run fills the cache)
  export Y5_TUNE_CACHE=/tmp/y5_tune_train.json
  [ -n "$Y5_SEED_TUNE_CACHE" ] && [ -f "$Y5_SEED_TUNE_CACHE" ] && cp "$Y5_SEED_TUNE_CACHE" "$Y5_TUNE_CACHE"
  timeout 300 python scripts/train_bench.py --steps 5 --warmup 3 > $OUT/train_bench.log 2>&1; tail -1 $OUT/train_bench.log
  rm -rf $OUT/trainprof
  (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trainprof" -o t -- python "$OLDPWD/scripts/train_bench.py" --steps 10 --warmup 3 > "$OUT/train_prof.log" 2>&1); echo "train prof rc=$?"
  f=$(find $OUT/trainprof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" $OUT/train_kernel_stats.csv && head -12 "$f" | cut -c1-150
  grep images/sec $OUT/train_prof.log | tail -1 > $OUT/train_line_under_rocprof.json
  rm -rf $OUT/trainprof
fi
