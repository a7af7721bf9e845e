#!/bin/bash
# Same-box A/B of bench.py between a worktree of an older commit (_ab_old/, built there) and this tree: ROUNDS (default 2) rounds of
# old, new with the same flags; a run that fails or exceeds its time limit ends the script (nothing more is started on the GPU).
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}; O=$R/gpurun_out; mkdir -p $O; cd $R
F="--steps ${STEPS:-5} --warmup 1 --no-cpu-baseline --no-live-pmc --through-trainer 0 --other-configs none"
P="import json,sys; d=json.loads(sys.stdin.read()); print(sys.argv[1], d['value'], d['ms_per_step'])"
run() { (cd $2 && timeout -k 10 400 python bench.py $F 2>/dev/null | tail -1 | python -c "$P" $1); }
for r in $(seq ${ROUNDS:-2}); do
  run old $R/_ab_old && run new $R || { echo "round $r: a run failed, stopping"; exit 1; }
done 2>&1 | tee $O/bench_ab.txt
