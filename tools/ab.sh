# A/B harness for experiments on the GPU box: bash tools/ab.sh "<pytest -k expr>" "<opt string 1>" "<opt string 2>" ...
set -e
export OUT=${OUT:-tool_out}   # output directory (logs, profiler output, kept libraries)
mkdir -p "$OUT"
K="$1"; shift
if [ -n "$K" ]; then
  python -m pytest tests/test_gpu_parity.py -x -q -m gpu -k "$K" > $OUT/ab_tests.log 2>&1 || { tail -40 $OUT/ab_tests.log; exit 1; }
  tail -1 $OUT/ab_tests.log
fi
i=0
for o in "$@"; do
  i=$((i+1))
  MVSIM_OPTIONS="$o" python bench.py --full --no-cpu-baseline --no-end-to-end --no-size-1024 --no-two-streams --no-compact-queue-leg > $OUT/ab_$i.log 2>&1 || { tail -5 $OUT/ab_$i.log; exit 1; }
  python - "$o" $OUT/ab_$i.log <<'PY'
import json, sys
for l in open(sys.argv[2]):
    if l.startswith("{"):
        d = json.loads(l); s = d["roofline"]["stage_ms"]
        print(f"[{sys.argv[1]}] {d['value']:.0f} Mvox/s  total {s['total_ms']:.3f}  rot {s['rotate_ms']:.3f} conv {s['convolve_ms']:.3f} (A {s['pass_a_ms']:.3f} B {s['pass_b_ms']:.3f} C {s['pass_c_ms']:.3f} D {s['pass_d_ms']:.3f} E {s['pass_e_ms']:.3f}) extract {s['extract_ms']:.3f}")
PY
done
