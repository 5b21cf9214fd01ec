#!/bin/bash
# GPU box: the full -m gpu suite, smoke(), and bench lines of BASELINE configs 1 / 2 / 4 and config 5's scenes of
# ranks 1 and 7 (round-end evidence)
set -e -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
OUT=${OFX_OUT:-$R/out}
mkdir -p $OUT
timeout -k 10 1000 python -u -m pytest tests/ -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gputest_full.log 2>&1
tail -3 $OUT/gputest_full.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1
tail -1 $OUT/smoke.log
for c in 1 2 4; do
  timeout -k 10 400 python bench.py --config $c --full --no-cpu-baseline --steps 30 > $OUT/bench_config$c.log 2>&1
  tail -1 $OUT/bench_config$c.log | cut -c1-200
done
for r in 1 7; do
  timeout -k 10 400 python bench.py --config 5 --scene-rank $r --full --no-cpu-baseline --steps 50 > $OUT/bench_config5_r$r.log 2>&1
  tail -1 $OUT/bench_config5_r$r.log | cut -c1-200
done
