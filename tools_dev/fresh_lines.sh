# The headline bench line and the 260 x 260 line, with their --full objects, as the first processes started on a box.
# usage: bash tools_dev/fresh_lines.sh [outdir]
O=${1:-bench_outputs/fresh}
mkdir -p "$O"
python bench.py --full --steps 40 2>/dev/null | tail -1 > "$O/bench_line_1gpu.json"
python bench.py --full --no-cpu-baseline --steps 40 --img-size 260 2>/dev/null | tail -1 > "$O/bench_config2_260.json"
python - "$O" <<'PY'
import json, sys
for f in ('bench_line_1gpu','bench_config2_260'):
    d=json.load(open('%s/%s.json'%(sys.argv[1], f))); print(f, d['value'], d['ms_per_step'], d['roofline']['frac'])
PY
