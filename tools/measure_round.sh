# Round measurement on the GPU box: PMC traffic (separate counter passes) -> kernel-trace stats -> full bench
# line with the CPU baseline (reads the PMC summary just written). Everything lands in $OFX_OUT (default out/; copied
# into profiles/ afterwards). Every GPU step has its own time limit; the script stops at the first failure.
set -e -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${TAG:-r05}
export OFX_OUT=${OFX_OUT:-$R/out}
OUT=$OFX_OUT
cd $R
mkdir -p $OUT
bash tools/pmc_traffic.sh
python tools/pmc_summary.py $OUT $OUT/${TAG}_pmc_traffic.json
cp $OUT/${TAG}_pmc_traffic.json profiles/${TAG}_pmc_traffic.json
bash tools/pmc_valu.sh
python tools/pmc_valu_summary.py $OUT/pmc_valu/run_counter_collection.csv $OUT/${TAG}_pmc_valu.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_final -o run -- python3 $R/bench.py --no-cpu-baseline > $OUT/bench_rocprof.log 2>&1
cd $R
grep '"metric"' $OUT/bench_rocprof.log | tail -1 > $OUT/${TAG}_bench_under_rocprof.json
python tools/kstats.py $OUT/prof_final/run_results.db --csv $OUT/${TAG}_bench_kernel_stats.csv > $OUT/kstats.txt
head -16 $OUT/kstats.txt
rm -rf $OUT/prof_final
timeout -k 10 900 python bench.py --full > $OUT/bench_full.log 2>&1
tail -1 $OUT/bench_full.log > $OUT/${TAG}_bench.json
cat $OUT/${TAG}_bench.json
timeout -k 10 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/bench_driver.log 2>&1
tail -1 $OUT/bench_driver.log > $OUT/${TAG}_bench_driver_form.json
cat $OUT/${TAG}_bench_driver_form.json
