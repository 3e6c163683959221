#!/bin/bash
# GPU round: build, parity tests, headline bench, rocprof kernel trace.  Every GPU
# step has its own time limit; a crash/timeout (rc >= 124 or signal) stops the script.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT_DIR=${OUT_DIR:-bench_out}  # logs and profiles (git-ignored)
mkdir -p $OUT_DIR
python -m leanfe_amd.build > $OUT_DIR/build.log 2>&1 || { echo build failed; exit 1; }
ok() { local rc=$1; [ $rc -eq 0 ] || [ $rc -eq 1 ]; }
if [ "${RUN_TESTS:-1}" = 1 ]; then
  eval "set -- ${PYTEST_ARGS:-}"  # shell-quoted extra arguments, e.g. PYTEST_ARGS="-k 'a or b'"
  timeout -k 10 ${TEST_TIMEOUT:-500} python -m pytest tests -m gpu -q -x -p no:cacheprovider "$@" > $OUT_DIR/pytest.log 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -3 $OUT_DIR/pytest.log
  ok $rc || exit $rc
fi
if [ "${RUN_BENCH:-1}" = 1 ]; then
  timeout -k 10 ${BENCH_TIMEOUT:-400} python bench.py --full ${BENCH_ARGS:-} > $OUT_DIR/bench.log 2>&1
  rc=$?; echo "bench rc=$rc"; tail -c 3000 $OUT_DIR/bench.log
  [ $rc -eq 0 ] || exit $rc
fi
if [ "${RUN_PROF:-0}" = 1 ]; then
  export TMPDIR=/tmp
  timeout -k 10 ${PROF_TIMEOUT:-400} rocprofv3 --kernel-trace --stats -d $OUT_DIR/prof -o run --output-format csv -- python bench.py ${PROF_ARGS:---full --steps 3 --warmup 1 --no-cpu} > $OUT_DIR/prof.log 2>&1
  rc=$?; echo "rocprof rc=$rc"; tail -5 $OUT_DIR/prof.log
fi
