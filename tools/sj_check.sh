#!/bin/bash
# On an MI355X: subjunc parity tests, then the C5 bench with its parity check and per-kernel times.
# Usage: tools/sj_check.sh [OUTDIR]   (default: a fresh temporary directory)
set -o pipefail
out=${1:-$(mktemp -d)}
mkdir -p $out
timeout -k 10 400 python -u -m pytest tests -m gpu -k "sj or subjunc or golden or pipelines" -x -q --timeout 120 --timeout-method thread > $out/tests.log 2>&1 || { tail -30 $out/tests.log; exit 1; }
tail -2 $out/tests.log
timeout -k 10 400 python -u bench.py --full --workload c5 --no-cpu --steps 3 > $out/c5.json 2> $out/c5.log || exit 1
python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(sys.argv[1],d['value'],d['parity_check'],{k:v['launch_ms'] for k,v in d['roofline']['kernels'].items()})" $out/c5.json
