#!/bin/bash
# Full measurement set for profiles/: parity tests, default bench (with CPU
# baseline), rocprofv3 kernel-trace stats, PMC FETCH/WRITE passes -> traffic.
# Each GPU step has its own time limit; a fault / timeout stops the script.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT_DIR=${OUT_DIR:-bench_out}  # logs and profiles (git-ignored)
mkdir -p $OUT_DIR
python -m leanfe_amd.build > $OUT_DIR/build.log 2>&1 || { echo build failed; exit 1; }
python -c "from oracle.altproj_c import build; build()" || exit 1
step() { local rc=$1 name=$2; echo "$name rc=$rc"; [ $rc -eq 0 ] || exit $rc; }
timeout -k 10 840 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread \
  > $OUT_DIR/pytest.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 $OUT_DIR/pytest.log; [ $rc -le 1 ] || exit $rc  # failures: still profile
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > $OUT_DIR/bench.log 2>&1
step $? bench; tail -c 2500 $OUT_DIR/bench.log
export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT_DIR/prof -o run --output-format csv \
  -- python bench.py --full --steps 5 --warmup 1 --no-cpu > $OUT_DIR/prof.log 2>&1
step $? rocprof
rm -rf $OUT_DIR/pmc
PASSES="fetch:FETCH_SIZE write:WRITE_SIZE" PMC_ARGS="--full --steps 2 --warmup 1 --no-cpu" bash tools/pmc.sh || exit $?
python tools/pmc_traffic.py $OUT_DIR/pmc $OUT_DIR/pmc_traffic.json --rows 50000000 --k 10 \
  --levels 100000,1000 --vcov HC1 > $OUT_DIR/pmc_traffic.log 2>&1
echo "traffic rc=$?"
