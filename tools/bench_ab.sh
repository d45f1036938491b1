#!/bin/bash
# bench.py of two builds of the project, alternating, one JSON line per run:
#   tools/bench_ab.sh PARENT_TREE [RUNS] > raw_bench_ab.jsonl
# PARENT_TREE: a checkout of the commit to compare against, with its library
# built in place; the other arm is this tree.  Headline step and policy mode of
# the four workloads; every run under its own time limit, and the first run
# that fails ends the measurement.
set -u
PAR=$(cd "$1" && pwd); RUNS=${2:-5}
NEW=$(cd "$(dirname "$0")/.." && pwd)
LOG=$(mktemp)
for rep in $(seq 1 "$RUNS"); do
  for W in invmgmt_backlog invmgmt_lostsales net_backlog newsvendor; do
    for M in step policy; do
      for A in parent new; do
        if [ $A = parent ]; then D=$PAR; else D=$NEW; fi
        ( cd "$D" && timeout -k 10 100 python bench.py --gpus 1 --workload $W --mode $M --steps 1500 --warmup 100 \
            --no-cpu-baseline > "$LOG" 2>&1 ) || { echo "FAILED $A $W $M" >&2; tail -20 "$LOG" >&2; exit 1; }
        tail -1 "$LOG" | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps(dict(rep=$rep, arm='$A', workload='$W', mode='$M', value=d['value'], kernel_us=d.get('roofline',{}).get('kernel_ms_mean',0)*1e3)))"
      done
    done
  done
done
