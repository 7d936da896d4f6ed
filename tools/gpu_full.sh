#!/bin/bash
# full GPU suite + smoke + the full bench (bench.py --full) on the current tree; logs under $OUT/
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}  # where the logs go
mkdir -p $OUT
TAG=${1:-r06}
timeout -k 10 1500 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/${TAG}_gputests.log 2>&1 || { tail -40 $OUT/${TAG}_gputests.log; exit 1; }
tail -3 $OUT/${TAG}_gputests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { tail -20 $OUT/${TAG}_smoke.log; exit 1; }
tail -2 $OUT/${TAG}_smoke.log
timeout -k 10 900 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -20 $OUT/${TAG}_bench.err; exit 1; }
python3 -c "
import json; d=json.loads(open('$OUT/${TAG}_bench.json').read().strip().splitlines()[-1])
print('fp32', d['value'], 'frac', d['roofline']['frac'], 'bf16', d.get('bf16', {}).get('value'), 'cpu', d.get('cpu_baseline', {}).get('value'))"
