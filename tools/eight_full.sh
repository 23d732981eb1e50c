#!/bin/bash
# stress: N ranks (default 8) of the headline bench on ONE device at the metric's own size (look-ahead regime, flag-ordered tail,
# chain_column_kernel all time-sliced between processes); stderr kept, every non-zero info and every warning counted
# usage: tools/eight_full.sh [ranks] [output directory (default: a new temporary one)]
cd "$(dirname "$0")/.."
n=${1:-8}
out=${2:-$(mktemp -d)}
mkdir -p $out
echo "output: $out"
d=$(mktemp -d)
BENCH_CFG3_POINTS=$n BENCH_CFG5_LADDERS=$n BENCH_CFG5_STEPS=4 GPMI_RDV_DIR=$d MASTER_PORT=29535 GPMI_DEBUG_INFO=1 \
  python bench.py --gpus $n --steps 3 --warmup 1 --full --no-cpu-baseline > $out/full_out.json 2> $out/full_err.txt
echo "rc=$?"
python - "$out" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1] + '/full_out.json').read().strip().splitlines()[-1])
print('n_gpus', d['n_gpus'], 'ms/step', round(d['ms_per_step'], 1), 'sharded:', d['sharded'].get('error', 'ok'),
      {k: round(v['seconds'], 2) for k, v in d['sharded'].items() if isinstance(v, dict)})
PY
echo "[gpmi] lines: $(grep -c '\[gpmi\]' $out/full_err.txt); warnings: $(grep -ci 'warn' $out/full_err.txt); timed out: $(grep -c 'timed out' $out/full_err.txt)"
grep -h "\[gpmi\]\|timed out\|Warning" $out/full_err.txt | sort | uniq -c | sort -rn | head -8
