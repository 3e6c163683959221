# end of round 6: full GPU suite, bench default line, config / preset lines with CPU baselines,
# rocprofv3 kernel stats, one-step traces of the 8-rank shard and configs 1 / 3
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT_DIR=${OUT_DIR:-bench_out}  # logs, profiles and traces (git-ignored)
mkdir -p $OUT_DIR
timeout -k 10 840 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread \
  > $OUT_DIR/pytest_final.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -2 $OUT_DIR/pytest_final.log; [ $rc -le 1 ] || exit $rc
timeout -k 10 300 python bench.py --full >$OUT_DIR/bench_default.log 2>&1 || { tail -3 $OUT_DIR/bench_default.log; exit 1; }
tail -c 300 $OUT_DIR/bench_default.log
bash tools/measure_lines.sh > $OUT_DIR/measure.log 2>&1 || { tail -3 $OUT_DIR/measure.log; exit 1; }
echo measure ok
bash tools/trace_run.sh > $OUT_DIR/trace.log 2>&1 || { tail -3 $OUT_DIR/trace.log; exit 1; }
for n in e8 c1 c3; do python tools/trace_gaps.py $OUT_DIR/tr/$n/run_kernel_trace.csv > $OUT_DIR/trace_gaps_$n.txt; tail -1 $OUT_DIR/trace_gaps_$n.txt; done
