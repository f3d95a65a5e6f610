#!/bin/bash
# Kernel-argument preload probe (scripts/probes/kernarg_preload_probe.hip): variants A .. E on the 64- and the
# 1440-workgroup grid, three alternations, every variant a process of its own under its own time limit.
# Builds the two binaries where they are missing (plain: A, B, D; with the preload option: C, E).
# Usage: bash scripts/gpu_kernarg_probe.sh [table file, default kernarg_preload_probe.txt in the repository root]
OUT=$(realpath -m "${1:-$(dirname "$0")/../kernarg_preload_probe.txt}")
cd "$(dirname "$0")/.." || exit 2
set -o pipefail
P=scripts/probes/kernarg_preload_probe
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -I include"
[ -x $P ] || hipcc $FLAGS -o $P $P.hip || exit 1
[ -x ${P}_pre ] || hipcc $FLAGS -mllvm -amdgpu-kernarg-preload-count=14 -o ${P}_pre $P.hip || exit 1
mkdir -p "$(dirname "$OUT")"
: > $OUT
for i in 1 2 3; do
    timeout -k 10 60 $P A ${REPLAYS:-300} | sed "s/^/r$i /" | tee -a $OUT &&
    timeout -k 10 60 $P B ${REPLAYS:-300} | sed "s/^/r$i /" | tee -a $OUT &&
    timeout -k 10 60 ${P}_pre C ${REPLAYS:-300} | sed "s/^/r$i /" | tee -a $OUT &&
    timeout -k 10 60 $P D ${REPLAYS:-300} | sed "s/^/r$i /" | tee -a $OUT &&
    timeout -k 10 60 ${P}_pre E ${REPLAYS:-300} | sed "s/^/r$i /" | tee -a $OUT || exit 1
done
# every variant computes the same tensor on each grid
for g in 64 1440; do
    n=$(grep "wgs *$g " $OUT | sed 's/.*hash \([0-9a-f]*\).*/\1/' | sort -u | wc -l)
    if [ "$n" != 1 ]; then echo "outputs differ on the $g-workgroup grid" | tee -a $OUT; exit 1; fi
done
echo "outputs equal across A .. E on both grids" | tee -a $OUT
