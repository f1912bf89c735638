OUT="${Y5_CHECK_OUT:-check_out}"; mkdir -p "$OUT" && OUT="$(cd "$OUT" && pwd)"; export Y5_TUNE_CACHE=/tmp/tune_ab.json
timeout 300 python bench.py --full --no-train --no-pipeline --no-cpu-baseline > /dev/null 2>&1
for i in 1 2; do for hb in 1 0; do
  Y5_HEAD_BRANCH=$hb timeout 300 python bench.py --full --no-train --no-pipeline --no-cpu-baseline --steps 100 > $OUT/bench_hb$hb.log 2>&1
  echo "branch=$hb $(tail -1 $OUT/bench_hb$hb.log | grep -o "\"value\": [0-9.]*\|\"forward_ms\": [0-9.]*\|\"conv_ms_per_step\": [0-9.]*" | tr "\n" " ")"
done; done
export TMPDIR=/tmp; R=$PWD
(cd /tmp && Y5_HEAD_BRANCH=0 timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_nb -o r -- python $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-train --no-pipeline > $OUT/prof_nb.log 2>&1)
t=$(find $OUT/prof_nb -name "*kernel_trace.csv" | head -1)
python scripts/rocprof_frac.py $t --gbytes 7.314 --out $OUT/prof_nb/rocprof_frac.json | head -9
grep "^{" $OUT/prof_nb.log | tail -1 | grep -o "\"forward_ms\": [0-9.]*\|\"conv_ms_per_step\": [0-9.]*\|\"frac\": [0-9.]*" | tr "\n" " "
find $OUT/prof_nb -name "*kernel_trace.csv" -delete
