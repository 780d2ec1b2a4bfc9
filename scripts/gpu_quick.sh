#!/bin/bash
# quick GPU check of the LANE_FMA family + the bench line (used while iterating on a kernel)
set -o pipefail
mkdir -p gpurun_out
timeout -k 10 600 python -m pytest tests/test_ub_gpu.py -x -q -m gpu 2>&1 | tail -15 > gpurun_out/quick_tests.txt
rc=$?
cat gpurun_out/quick_tests.txt
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full | tail -1 | python -c '
import json, sys
d = json.loads(sys.stdin.read())
for k in ("value", "ms_per_step", "kernel_ms", "roofline", "alu", "max_abs_du_vs_dlib", "vs_bit_exact", "pipelined"):
    print(k, d.get(k))
'
