#!/bin/bash
# A/B on ONE box, arms alternating in every repetition.  An arm is either
#   label=lib.so[:ENV=VAL...]   a library build under lmx/ of THIS tree (LMX_LIB): bench.py --full --no-cpu-baseline, it reads the
#                               roofline leg; or
#   label=DIR[:ENV=VAL...]      a whole tree (its own library and Python, e.g. an export of the parent commit with its library built):
#                               the headline, python bench.py --gpus 1, run inside DIR.
# usage: [REPS=5] bash tools/ab_bench.sh out_name arm arm ...     (REPS defaults to 2; the first arm is the baseline of the summary)
set -u
OUT=gpurun_out/$1; shift
mkdir -p $(dirname $OUT)
: > $OUT
for rep in $(seq 1 ${REPS:-2}); do
for arm in "$@"; do
  label=${arm%%=*}; rest=${arm#*=}
  what=${rest%%:*}; envs=""
  if [[ "$rest" == *:* ]]; then envs=$(echo "${rest#*:}" | tr ':' ' '); fi
  if [ -d "$what" ]; then
    line=$(set -o pipefail; cd "$what" && env $envs timeout -k 10 300 python bench.py --gpus 1 2>/dev/null | tail -1); rc=$?
    if [ $rc -ne 0 ]; then echo "$label rep$rep rc=$rc: stopping" | tee -a $OUT; exit $rc; fi  # nothing more on a GPU after a failed run
    echo "$label rep$rep rc=$rc $(echo "$line" | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print("value", round(d["value"],2), "ms_per_step", round(d["ms_per_step"],3))')" | tee -a $OUT
  else
    line=$(env $envs LMX_LIB=$PWD/vision-sam3-yolo-lameless_amd/lmx/$what timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 8 --warmup 2 2>/dev/null | tail -1)
    echo "$label rep$rep $(echo "$line" | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print("value", round(d["value"],1), "ms/step", round(d["ms_per_step"],2), "gemm TF", round(d["roofline"]["achieved"],1), "serial", d["roofline"]["measured_on"][-28:])')" | tee -a $OUT
  fi
done
done
# per arm: mean, min, max and spread of `value`; every later arm against the first in units of the first arm's own spread
python - $OUT <<'EOF' | tee -a $OUT
import sys
runs = {}
for ln in open(sys.argv[1]):
    w = ln.split()
    if "value" in w:
        runs.setdefault(w[0], []).append(float(w[w.index("value") + 1]))
base = None
for label, v in runs.items():
    mean, spread = sum(v) / len(v), max(v) - min(v)
    print(f"{label:8s} runs {len(v)}  mean {mean:.2f}  min {min(v):.2f}  max {max(v):.2f}  spread (max - min) {spread:.2f}")
    if base is None:
        base = (label, mean, spread, max(v))
    else:
        print(f"{label} - {base[0]}: {mean - base[1]:+.2f} frames/s ({100 * (mean - base[1]) / base[1]:+.2f} %), "
              f"{(mean - base[1]) / base[2] if base[2] else float('inf'):.1f} x {base[0]}'s own spread; slowest {label} {min(v):.2f} "
              f"{'>' if min(v) > base[3] else '<='} fastest {base[0]} {base[3]:.2f}")
EOF
