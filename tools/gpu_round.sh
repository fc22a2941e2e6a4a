#!/bin/bash
# One GPU visit: the whole -m gpu suite (not -x: every failure is wanted), the default bench line (--full) and the track workload.
#   tools/gpu_round.sh <tag> [dir]      -> <dir>/<tag>_{pytest.log,bench_default.json,bench_track.json}   (dir: results/)
cd "$(dirname "$0")/.."
TAG=${1:-r03}
OUT=${2:-results}
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -q -m gpu ${PYTEST_ARGS:-} > "$OUT/${TAG}_pytest.log" 2>&1
echo "pytest rc=$?"; tail -15 "$OUT/${TAG}_pytest.log"
timeout 600 python bench.py --full > "$OUT/${TAG}_bench_default.json" 2> "$OUT/${TAG}_bench_default.err"; echo "bench rc=$?"
python - <<PY
import json
d=json.load(open("$OUT/${TAG}_bench_default.json"))
print("default:", round(d["value"],1), "pairs/s", round(d["ms_per_step"],3), "ms; points-only", round(d["config"]["points_only_pairs_per_s"],1), "roofline", round(d["roofline"]["frac"],3), "cpu", round(d["cpu_baseline"]["value"],2))
print({k: round(v["ms_per_step"],3) for k,v in d["stages"].items()})
PY
timeout 600 python bench.py --workload track > "$OUT/${TAG}_bench_track.json" 2> "$OUT/${TAG}_bench_track.err"; echo "track rc=$?"
python -c "import json; d=json.load(open('$OUT/${TAG}_bench_track.json')); print('track:', round(d['value'],1), d['unit'], round(d['ms_per_step'],3), 'ms', d['config'].get('matches_mean'), d['config'].get('lines_mean'))"
