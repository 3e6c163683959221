#!/bin/bash
# Same-box A/B of two engine builds: tools/ab_old.so (baseline) vs the in-tree library.
#   KEYS="part_scatter" ROUNDS=3 bash tools/ab_lib.sh
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT_DIR=${OUT_DIR:-bench_out}  # logs (git-ignored)
mkdir -p $OUT_DIR
for r in $(seq 1 ${ROUNDS:-3}); do
  for lib in tools/ab_old.so leanfe_amd/liblfe_hip.so; do
    LEANFE_HIP_LIB=$PWD/$lib timeout -k 10 120 python bench.py --full --no-cpu --steps ${STEPS:-10} --warmup 5 > $OUT_DIR/ab.log 2>&1
    rc=$?; [ $rc -eq 0 ] || { echo "$lib rc=$rc"; tail -3 $OUT_DIR/ab.log; exit $rc; }
    python - "$lib" "${KEYS:-}" "$OUT_DIR/ab.log" <<'PY'
import json, sys
lib, keys = sys.argv[1], [k for k in sys.argv[2].split(",") if k]
d = json.loads([l for l in open(sys.argv[3]) if l.startswith("{")][-1])
ks = d["kernels_ms"]
print(f"{lib:>28}: {d['ms_per_step']:.3f} ms/step  " + "  ".join(f"{k}={ks[k][0]:.4f}" for k in keys if k in ks))
PY
  done
done
