#!/bin/bash
# HBM traffic of the rollout kernel from the L2 memory-side counters, per MI355X_MICROARCH.md §HBM:
# FETCH_SIZE and WRITE_SIZE in SEPARATE --pmc passes (with --kernel-trace only), calibrated on a plain float4
# copy of an obs-sized buffer (known bytes, same 16-byte-per-lane access width), gfx950 FETCH_SIZE x2.
# Usage (GPU box, repo root): bash scripts/pmc_traffic.sh <tag>   -> gpurun_out/<tag>/pmc_traffic.json
TAG=${1:-pmc}
OUT=gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
[ -x scripts/micro/copybench ] || make -s -C scripts/micro copybench
# the hash of the kernel sources these passes measure, stamped HERE, at measurement time (pmc_traffic.py carries it into the JSON;
# bench.py refuses the bytes of other code)
python -c "import json; from env_build_amd import build as b; json.dump({k: b.kernel_hash(k) for k in b.KERNEL_SOURCES}, open('$OUT/kernel_hash.json', 'w'))"
# every pass under a time limit of its own; the first pass that fails, faults or runs out of time ends the script
run() { local t=$1 name=$2; shift 2; timeout -k 10 $t "$@" > $OUT/$name.log 2>&1 || { echo "$name failed (exit $?): $OUT/$name.log"; exit 1; }; }
for c in FETCH_SIZE WRITE_SIZE; do
  run 900 bench_$c rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/bench_$c -o p -- python bench.py --steps 50 --warmup 25 --no-cpu-baseline --no-side
  run 300 copy_$c rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/copy_$c -o p -- scripts/micro/copybench calib
  run 600 envstep_$c rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/envstep_$c -o p -- python bench.py --env-step
  run 600 f16_$c rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/f16_$c -o p -- python scripts/time_rollout.py --n-veh 64 --f16 --iters 60
done
python scripts/pmc_traffic.py $OUT | tee $OUT/pmc_traffic.txt
