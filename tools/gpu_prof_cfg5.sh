#!/bin/bash
# cfg5 at its full size (8192 envs, knuffingen, 480x640 rgb: 7.55 GB of observations per step): bench line, kernel stats, PMC
R=$GRAFT_REPO_ROOT; tag=r02_cfg5
O=$R/bench_out; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
A="--workload cfg5 --steps 64 --warmup 8 --preroll-ms 50"
timeout -k 10 400 python3 $R/bench.py --full $A --cpu-budget 4000 > $O/bench_${tag}.json 2> $O/bench_${tag}.err || { tail -3 $O/bench_${tag}.err; exit 1; }
cut -c1-900 $O/bench_${tag}.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${tag} -- python3 $R/bench.py $A --no-cpu-baseline > $O/prof_${tag}.log 2>&1 || { tail -3 $O/prof_${tag}.log; exit 1; }
grep -h "tc_" $O/prof_${tag}/*/*_kernel_stats.csv | cut -c1-220
i=0
for set in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY" "FETCH_SIZE" "WRITE_SIZE"; do
  i=$((i+1))
  timeout -k 10 400 rocprofv3 --pmc $set --output-format csv -d $O/pmc_${tag}/p$i -- python3 $R/bench.py --workload cfg5 --steps 16 --warmup 4 --preroll-ms 0 --no-cpu-baseline > $O/pmc_${tag}_p$i.log 2>&1 || echo "pmc pass $i failed"
done
