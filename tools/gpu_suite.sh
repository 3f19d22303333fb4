#!/bin/bash
# GPU session script: the whole -m gpu suite (no -x: every failure listed), then a default bench
# line with its side measurements (--full).  Output under $OUT/<tag>_* (default bench_out/).
# Usage: tools/gpu_suite.sh TAG [pytest -k expression]
set -o pipefail
TAG=${1:-s}
K=${2:-}
OUT=${OUT:-bench_out}
cd "${GRAFT_REPO_ROOT:-.}"
mkdir -p $OUT
if [ -n "$K" ]; then KARG=(-k "$K"); else KARG=(); fi
timeout -k 10 1000 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread -p no:cacheprovider \
  "${KARG[@]}" > $OUT/${TAG}_pytest.log 2>&1
rc=$?
tail -5 $OUT/${TAG}_pytest.log
grep -E "FAILED|ERROR" $OUT/${TAG}_pytest.log | head -40
# a fault / abort / timeout ends the session here (no further GPU work)
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest rc=$rc: stopping"; exit $rc; fi
timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
echo "bench rc=$?"
cat $OUT/${TAG}_bench.json | cut -c1-600
# optional: per-kernel timings (tools/bench_kernels.py modes, e.g. "episode hole")
if [ -n "$3" ]; then
  timeout -k 10 400 python tools/bench_kernels.py $3 > $OUT/${TAG}_kernels.jsonl 2> $OUT/${TAG}_kernels.err
  echo "kernels rc=$?"
  cut -c1-300 $OUT/${TAG}_kernels.jsonl
fi
