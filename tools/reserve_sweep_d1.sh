mkdir -p gpurun_out/rs
for r in 96 0 64 128 160 192 256 96; do
  timeout 300 python bench.py --full --variant pca --mode direct1 --stream-reserve $r --cpu-seconds 0 --no-host-clouds --seq-frames 0 --config4-pairs 0 --no-other-configs 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d['roofline']; t=d.get('tolerance_mode') or {}
print('reserve $r', 'stream', d['value'], 'sync', d['value_synchronous'], 'ms', d['ms_per_step'], 'launch', r['avg_launch_us'], 'build', r['build_ms_per_step'], '| tol stream', t.get('value_tolerance_mode_streamed'), 'sync', t.get('value_tolerance_mode_synchronous'))"
done > gpurun_out/rs/out.txt 2>&1
cat gpurun_out/rs/out.txt
