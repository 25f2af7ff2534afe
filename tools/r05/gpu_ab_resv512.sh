# DEV TOOL (GPU box): reservoir512 (two workgroups per CU) and reservoir (one), shipped library vs lamejs_amd/lib/variants/*.so, alternating
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/r05_ab_resv; mkdir -p $O
cd $R
run() { timeout 200 python bench.py --full --no-extras --cpu-seconds 0 --steps 4 --warmup 1 --check-frames 0 --config $2 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$1', 'config $2', 'ms_per_step', d['ms_per_step'], 'frames/s', d['value'], 'bit_exact_full', d['config']['bit_exact_full'])"; }
{
for rep in 1 2; do
  for c in reservoir512 reservoir; do
    unset LAMEJS_HIP_LIB; run shipped $c
    for v in lamejs_amd/lib/variants/*.so; do export LAMEJS_HIP_LIB=$R/$v; run $(basename $v .so) $c; done
  done
done
} 2>&1 | tee $O/ab.txt
