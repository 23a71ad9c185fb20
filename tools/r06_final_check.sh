set -x
cd "$(dirname "$0")/.."
O=${OUT:-bench_runs/r06z}; mkdir -p $O
S=$SECONDS
timeout 1500 python -m pytest tests -x -q -m gpu > $O/pytest_gpu.txt 2>&1; echo "pytest rc $? in $((SECONDS-S)) s" >> $O/pytest_gpu.txt
tail -5 $O/pytest_gpu.txt
S=$SECONDS
timeout 900 python bench.py --full > $O/bench.json 2> $O/bench.err; echo "bench rc $? in $((SECONDS-S)) s"
O=$O python - <<'PY'
import json, os
j=json.loads(open(os.environ['O'] + '/bench.json').read().strip().splitlines()[-1])
print({k:j[k] for k in ('metric','value','ms_per_step')}, j['roofline'])
PY
