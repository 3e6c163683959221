set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
OUT_DIR=${OUT_DIR:-bench_out}  # logs and traces (git-ignored)
mkdir -p $OUT_DIR/tr
for c in "e8:--emulate-rank 0/8" "c1:--config 1" "c3:--config 3"; do
  n=${c%%:*}; args=${c#*:}
  timeout -k 10 200 rocprofv3 --kernel-trace --memory-copy-trace -d $OUT_DIR/tr/$n -o run --output-format csv -- python bench.py --no-cpu --no-h2d --no-prof --steps 6 --warmup 3 --runs 1 $args > $OUT_DIR/tr/$n.log 2>&1 || { echo "$n failed"; tail -5 $OUT_DIR/tr/$n.log; exit 1; }
  echo "$n ok"; tail -c 300 $OUT_DIR/tr/$n.log
done
# host side: HIP runtime API calls beside the kernels of the 8-rank shard (no counters)
timeout -k 10 200 rocprofv3 --kernel-trace --hip-runtime-trace -d $OUT_DIR/tr/e8api -o run --output-format csv -- python bench.py --no-cpu --no-h2d --no-prof --steps 4 --warmup 3 --runs 1 --emulate-rank 0/8 > $OUT_DIR/tr/e8api.log 2>&1 || { echo "e8api failed"; tail -5 $OUT_DIR/tr/e8api.log; exit 1; }
echo "e8api ok"
