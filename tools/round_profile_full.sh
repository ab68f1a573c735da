#!/bin/bash
# Round-end evidence: FRS profile + PMC passes (round_profile.sh), the full bench line,
# and the sparse-conv GEMM probe under rocprofv3 kernel-trace -> $OUT_DIR/r02s4/
# (OUT_DIR: an absolute path; default out/ in the tree)
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT_DIR=${OUT_DIR:-$PWD/out}
OUT=$OUT_DIR/r02s4
TAG=r02s4 bash tools/round_profile.sh || exit 1
timeout -k 10 400 python bench.py --full > "$OUT/full_bench.log" 2>&1 || { echo "bench rc=$?"; exit 1; }
tail -1 "$OUT/full_bench.log" | cut -c1-300
R=$(pwd); export TMPDIR=/tmp
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/sc" -o run --output-format csv \
    -- python3 "$R/tools/gemm_probe.py" > "$OUT/gemm_probe.log" 2>&1) || { echo "probe rc=$?"; exit 1; }
grep cin "$OUT/gemm_probe.log"
