#!/bin/bash
# bench line incl. the new extras + the two-rank rehearsals
out=${1:?usage: tools/gpu_r3c.sh OUTDIR}
export out
mkdir -p "$out"
timeout -k 10 500 python bench.py --full --steps 20 --warmup 3 > "$out"/bench_cycle.json 2> "$out"/bench_cycle.err || { tail -20 "$out"/bench_cycle.err; exit 1; }
python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ['out'], 'bench_cycle.json')).read().strip().splitlines()[-1])
print("value %.0f ms/step %.3f median kernel %.3f | hinted %.3f ms | cpu %.0f dX %.2e" % (
    d['value'], d['ms_per_step'], d['median_kernel_ms'], d['schedule_hint']['hinted_ms'], d['cpu_baseline']['value'], d['cpu_baseline']['max_abs_dX_vs_gpu']))
print("roofline frac %.4f" % d['roofline']['frac'])
print("pipelined:", json.dumps({k: v for k, v in d.get('pipelined_budget', {}).items() if k != 'note'}))
print("c5:", json.dumps(d.get('c5'))[:1500])
PY
timeout -k 10 900 python -m pytest tests/test_bench_ranks.py -m gpu -x -q > "$out"/bench_ranks.log 2>&1; rc=$?
tail -15 "$out"/bench_ranks.log
exit $rc
