#!/bin/bash
# Round-3 profile on the GPU box: kernel-trace stats of bench.py --full with the JSON line printed inside that
# run, SQ / HBM counters of the step's kernels (tools/step_pmc.sh -> step_valu.json), HBM counters of the graded kernel
# (-> osc_traffic.json, both carry the hash of the kernel sources), the FilteredNoise kernel alone (tools/noise_pmc.sh).
set -eu          # the first step that fails, faults or times out ends the script: nothing more starts on the card
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=$R/gpurun_out/prof_r03
mkdir -p $OUT
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt -o bench -- python $R/bench.py --full --steps 10 --warmup 2 > $OUT/bench_under_rocprof.log 2>&1
grep "^{\"metric" $OUT/bench_under_rocprof.log > $OUT/bench_under_rocprof.json
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o p -- python $R/tools/bench_kernels.py --which osc --spans 1 --reps 2 > $OUT/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o p -- python $R/tools/bench_kernels.py --which osc --spans 1 --reps 2 > $OUT/pmc_write.log 2>&1
cd $R
python tools/osc_traffic.py $(find $OUT/pmc_fetch -name '*counter_collection.csv' | head -1) $(find $OUT/pmc_write -name '*counter_collection.csv' | head -1) $OUT/osc_traffic.json
python tools/pmc_summary.py $(find $OUT/pmc_fetch -name '*counter_collection.csv' | head -1) "osc_kernel<1, false" > $OUT/osc_pmc.txt
python tools/pmc_summary.py $(find $OUT/pmc_write -name '*counter_collection.csv' | head -1) "osc_kernel<1, false" >> $OUT/osc_pmc.txt
bash tools/step_pmc.sh r03 > $OUT/step_pmc.log 2>&1
cp gpurun_out/step_pmc_r03/summary.txt $OUT/step_pmc_summary.txt
cp gpurun_out/step_pmc_r03/step_valu.json $OUT/step_valu.json
cp $(find $OUT/kt -name '*kernel_stats.csv' | head -1) $OUT/bench_kernel_stats.csv
bash tools/noise_pmc.sh prof_r03_noise 8 > /dev/null 2>&1
cp gpurun_out/prof_r03_noise/summary.txt $OUT/noise_pmc.txt
# the bench line with the fresh counters in place
cp $OUT/step_valu.json $OUT/osc_traffic.json profiles/
timeout -k 10 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err
find $OUT -name "*.csv" ! -name "bench_kernel_stats.csv" -delete
ls $OUT
