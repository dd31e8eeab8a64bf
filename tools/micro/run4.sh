OUT=${1:?usage: bash tools/micro/run4.sh OUT_DIR}
mkdir -p $OUT
python -m pytest tests/test_gpu_graph.py tests/test_gpu_hidden.py -x -q > $OUT/t5.log 2>&1; tail -4 $OUT/t5.log
for r in 1 2; do
for m in "--one-stream --no-graph" "--two-streams --no-graph" "--two-streams --graph" "--one-stream --no-graph --keep-dead-grads"; do
  python bench.py --full --no-cpu-baseline --no-extra $m 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$m', round(d['ms_per_step'],4), round(d['ms_per_step_median_events'],4), 'host', round(d['host_enqueue_ms_median'],3), 'bwd', round(d['roofline']['avg_launch_ms']*1000,1), 'fwd', round(d['roofline_mfma']['avg_launch_ms']*1000,1), round(d['step_flops_frac_of_peak'],4))"
done; done 2>&1 | tee $OUT/modes2.log
python bench.py --full --no-cpu-baseline --two-streams --graph > $OUT/b3.json 2> $OUT/b3.err; tail -c 1800 $OUT/b3.json
