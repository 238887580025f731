# usage: bash tools/prof_driver.sh    (GPU box)
# rocprofv3 --kernel-trace --stats of the full benchmark run
# (python3 bench.py --gpus 1 --steps 20 --warmup 5 --full), so that the average duration of the dominant
# kernel can be compared with roofline.launch_us of the line that same run printed.
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
mkdir -p bench_out
rm -rf bench_out/prof_driver
rocprofv3 --kernel-trace --stats --output-format csv -d bench_out/prof_driver -- python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > bench_out/prof_driver.log 2>&1
find bench_out/prof_driver -name "*kernel_stats.csv" -exec cp {} bench_out/stats_driver.csv \;
find bench_out/prof_driver -name "*_kernel_trace.csv" -delete
find bench_out/prof_driver -name "*.db" -delete
grep '^{"metric"' bench_out/prof_driver.log > bench_out/bench_under_rocprof_driver.json
cut -c1-400 bench_out/bench_under_rocprof_driver.json
head -8 bench_out/stats_driver.csv | cut -c1-220
