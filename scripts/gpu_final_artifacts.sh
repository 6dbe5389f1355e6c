set -x
export OUT=${OUT:-$PWD/prof_out}; mkdir -p $OUT
python bench.py --full > $OUT/r6f_bench.json 2> $OUT/r6f_bench.err
python bench.py --full --workload det800 --no-cpu-baseline > $OUT/r6f_bench_det800.json 2>> $OUT/r6f_bench.err
python bench.py --full --workload swinb1024 --no-cpu-baseline > $OUT/r6f_bench_swinb1024.json 2>> $OUT/r6f_bench.err
bash scripts/gpu_prof_graph.sh r6f
bash scripts/gpu_prof_bench.sh r6f
bash scripts/gpu_pmc.sh r6f
ls $OUT | grep r6f
