#!/bin/bash
# kernel traces of the merged and the two-call schedule (16 episodes each) -> timeline_gaps / overlap_trace summaries
out=${1:-gpurun_out/trace_merge}
mkdir -p $out
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
for m in 1 0; do
  LMKD_MERGE=$m LMKD_TIMED_EVENTS=0 rocprofv3 --kernel-trace --output-format csv -d $R/$out/m$m -- python3 $R/bench.py --steps 48 --warmup 4 --no-cpu-baseline --no-other-modes --full --roofline-episodes 1 > $R/$out/m$m.json 2> $R/$out/m$m.err
  f=$(find $R/$out/m$m -name "*kernel_trace.csv" | head -1)
  echo "== LMKD_MERGE=$m  $f"
  python3 $R/tools/timeline_gaps.py $f 0.15 0.4
  python3 $R/tools/overlap_trace.py $f 0.15 0.4 | head -24
  rm -rf $R/$out/m$m
done
