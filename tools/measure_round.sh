#!/bin/bash
# The measurement set behind DESIGN.md / profiles/ (run on the GPU box from the repo root):
#   bash tools/measure_round.sh <tag> <output dir>          e.g. r02 out
# for each arithmetic mode (f32 = the headline, bf16x3 and bf16 = the labelled sub-records):
#   1. rocprofv3 --kernel-trace --stats over the bench command (eager launches, so every kernel is traced)
#   2. two PMC passes (FETCH_SIZE, WRITE_SIZE: they do not fit one pass) over the same command, counters only
#   3. tools/traffic_summary.py -> <output dir>/<tag>_traffic_<mode>.json (bytes per launch and kernel, gfx950 correction applied)
# then 4. the --full bench line (fp32 headline + split-bf16 and bf16 sub-records, HIP-graph replay, probe, CPU baseline)
tag=${1:-r04}
mkdir -p "${2:?usage: tools/measure_round.sh <tag> <output dir>}" || exit 1
OUT=$(cd "$2" && pwd)
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}
for prec in f32 bf16x3 bf16; do
  BENCH="python3 $R/bench.py --no-cpu-baseline --no-probe --graph 0 --sub-record 0 --precision $prec"
  (cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_${prec}_stats -- $BENCH --steps 5 --warmup 2 > $OUT/${tag}_${prec}_stats.log 2>&1) || exit 1
  (cd /tmp && rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${tag}_${prec}_fetch -- $BENCH --steps 2 --warmup 1 > $OUT/${tag}_${prec}_fetch.log 2>&1) || exit 1
  (cd /tmp && rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${tag}_${prec}_write -- $BENCH --steps 2 --warmup 1 > $OUT/${tag}_${prec}_write.log 2>&1) || exit 1
  python3 $R/tools/traffic_summary.py $OUT/${tag}_${prec}_fetch $OUT/${tag}_${prec}_write $OUT/${tag}_traffic_${prec}.json || exit 1
  cp $(ls $OUT/${tag}_${prec}_stats/*/*kernel_stats.csv | head -1) $OUT/${tag}_kernel_stats_${prec}.csv
done
python3 $R/bench.py --full > $OUT/${tag}_bench.log 2>&1
tail -1 $OUT/${tag}_bench.log | cut -c1-600
