#!/bin/bash
# One GPU visit, parameterised (replaces the per-visit scripts of round 4):
#   bash scripts/gpu_visit.sh <tag> [step ...]     steps: tests[:<pytest -k expr>] smoke bench bench_full reduce_ab[:cfgs] py:<script+args>
# Everything lands under $OUT/<tag>_* (OUT=out by default).  Each step runs under its own `timeout`.
set -u
TAG=$1; shift
OUT=${OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
for step in "$@"; do
  name=${step%%:*}; arg=""; [ "$step" != "$name" ] && arg=${step#*:}
  case $name in
    tests)
      if [ -n "$arg" ]; then timeout 1500 python -m pytest tests -m gpu -q -rfs -p no:cacheprovider -k "$arg" > $OUT/${TAG}_pytest_gpu.log 2>&1
      else timeout 1500 python -m pytest tests -m gpu -q -rfs -p no:cacheprovider > $OUT/${TAG}_pytest_gpu.log 2>&1; fi
      echo "tests rc=$?"; tail -15 $OUT/${TAG}_pytest_gpu.log;;
    smoke) timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1; echo "smoke rc=$?"; tail -1 $OUT/${TAG}_smoke.log;;
    bench) timeout 600 python bench.py --full --no-cpu-baseline $arg > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?"
      python scripts/bench_digest.py $OUT/${TAG}_bench.json;;
    bench_full) timeout 900 python bench.py --full $arg > $OUT/${TAG}_bench_full.json 2> $OUT/${TAG}_bench_full.err; echo "bench_full rc=$?"
      python scripts/bench_digest.py $OUT/${TAG}_bench_full.json;;
    reduce_ab) timeout 600 python scripts/reduce_ab.py $arg 2>&1 | grep -v amdgpu.ids | tee $OUT/${TAG}_reduce_ab.txt;;
    py) s=${arg%% *}; timeout 900 python scripts/$arg 2>&1 | grep -v amdgpu.ids | tee $OUT/${TAG}_$(basename $s .py).txt;;
    *) echo "unknown step $step";;
  esac
done
