# full GPU suite on the final library, then kernel + runtime traces of the 8-rank shard and configs
# 1 and 3 (trace_gaps summaries for profiles/)
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT_DIR=${OUT_DIR:-bench_out}  # logs and traces (git-ignored)
mkdir -p $OUT_DIR
timeout -k 10 840 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread \
  > $OUT_DIR/pytest_final.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 $OUT_DIR/pytest_final.log; [ $rc -le 1 ] || exit $rc
rm -rf $OUT_DIR/tr
bash tools/trace_run.sh > $OUT_DIR/trace.log 2>&1; echo "trace rc=$?"
for n in e8 c1 c3; do python tools/trace_gaps.py $OUT_DIR/tr/$n/run_kernel_trace.csv > $OUT_DIR/trace_gaps_$n.txt; tail -1 $OUT_DIR/trace_gaps_$n.txt; done
