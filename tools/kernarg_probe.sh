# does placing kernel arguments in device memory (HIP_FORCE_DEV_KERNARG) change the dependent-launch cost?
for v in 0 1; do
  HIP_FORCE_DEV_KERNARG=$v python bench.py --full --no-cpu-baseline 2>/dev/null | tail -1 | python -c "
import json, sys
d = json.loads(sys.stdin.read())
print('HIP_FORCE_DEV_KERNARG=$v', d['ms_per_step'], d['roofline']['avg_launch_us'], d['roofline']['single_block_kernel']['avg_launch_us'], d['kernels']['call_us'])
"
done
