# VALU instructions per wave of the Poisson kernels for experiment builds: bash tools/attribute_valu.sh "<cflags 1>" "<cflags 2>" ...
set -e
export OUT=${OUT:-tool_out}   # output directory (logs, profiler output, kept libraries)
mkdir -p "$OUT"
for f in "$@"; do
  MVSIM_EXTRA_CFLAGS="-DMVSIM_DEV_ATTRIBUTION $f" python -c "import importlib; b = importlib.import_module('multiview-simulation_amd.build'); b.build(force=True)"
  echo "[$f]"
  bash tools/pmc_i.sh "" > $OUT/pi.txt 2>&1 || { tail -5 $OUT/pi.txt; exit 1; }
  grep -i "extract\|resolve" $OUT/pi.txt | cut -c1-40,88-200
  python bench.py --full --no-cpu-baseline --no-end-to-end --no-size-1024 --no-two-streams 2>/dev/null | python -c "
import json,sys
for l in sys.stdin:
    if l.startswith('{'):
        s=json.loads(l)['roofline']['stage_ms']; print('   extract_ms', s['extract_ms'], 'total', s['total_ms'])
"
done
# leave the product build behind, not the last experiment
python -c "import importlib; b = importlib.import_module('multiview-simulation_amd.build'); b.build(force=True)"
