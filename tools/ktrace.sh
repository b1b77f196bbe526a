# per-kernel average durations of the bench under rocprofv3 --kernel-trace --stats: bash tools/ktrace.sh "<MVSIM_OPTIONS>"
set -e
export OUT=${OUT:-tool_out}   # output directory (logs, profiler output, kept libraries)
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
export MVSIM_OPTIONS="$1"
rm -rf $OUT/kt && mkdir -p $OUT/kt
rocprofv3 --kernel-trace --stats -d $OUT/kt -o run -- python3 bench.py --full --no-cpu-baseline --no-end-to-end --no-size-1024 --no-two-streams > $OUT/kt.log 2>&1
python3 tools/kstats.py $OUT/kt 14
rm -rf $OUT/kt
