#!/bin/bash
# kernel timeline of the predict pass (bench.py --full, few training steps): $OUT/*/*kernel_trace.csv
out=${OUT:-profile_out/tk_tl}
export TMPDIR=/tmp
rm -rf $out && mkdir -p $out
rocprofv3 --kernel-trace --output-format csv -d $out -- python3 bench.py --full --steps 5 --warmup 5 --no-cpu-baseline --no-prof --topk-chunk ${1:-131072} > $out.log 2>&1
ls $out/*/ | head
