set -e
export OUT=${OUT:-tool_out}   # output directory (logs, profiler output, kept libraries)
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
export MVSIM_OPTIONS="$1"
rm -rf $OUT/pi && mkdir -p $OUT/pi
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR -d $OUT/pi -o run -- python3 bench.py --full --no-cpu-baseline --no-end-to-end --no-size-1024 --no-two-streams --no-dense-leg --serial --steps 1 --warmup 1 > $OUT/pi.log 2>&1
python3 tools/pmc_insts.py $OUT/pi
rm -rf $OUT/pi
