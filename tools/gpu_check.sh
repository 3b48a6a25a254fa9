#!/bin/bash
# One GPU session: parity tests, smoke, bench, rocprof kernel trace.  Stops at the first
# crash/timeout (exit codes other than 0/1 from pytest).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
RESULTS=${RESULTS:-out}
mkdir -p $RESULTS
export TMPDIR=/tmp
(command -v go && go version) > $RESULTS/probe.log 2>&1; nproc >> $RESULTS/probe.log; lscpu | head -20 >> $RESULTS/probe.log
rocm-smi --showproductname >> $RESULTS/probe.log 2>&1
TESTS=${TESTS:-tests}
timeout -k 10 ${TEST_TIMEOUT:-900} python -u -m pytest $TESTS -m gpu -x -v --timeout 300 --timeout-method thread > $RESULTS/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc"
tail -5 $RESULTS/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stopping after pytest rc=$rc"; exit $rc; fi
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > $RESULTS/smoke.log 2>&1 || { echo "smoke failed"; cat $RESULTS/smoke.log | tail -20; exit 3; }
cat $RESULTS/smoke.log
timeout -k 10 300 python -u bench.py ${BENCH_ARGS:---full} > $RESULTS/bench.log 2>&1 || { echo "bench failed"; tail -20 $RESULTS/bench.log; exit 4; }
if [ -n "$BENCH2" ]; then timeout -k 10 300 python -u bench.py $BENCH2 > $RESULTS/bench2.log 2>&1 || { echo "bench2 failed"; tail -20 $RESULTS/bench2.log; exit 4; }; cat $RESULTS/bench2.log; fi
cat $RESULTS/bench.log
if [ -n "$PROFILE" ]; then
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $RESULTS/prof -o run --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu > $RESULTS/prof.log 2>&1 || { echo "rocprof failed"; tail -20 $RESULTS/prof.log; exit 5; }
  find $RESULTS/prof -name '*stats*' | head
fi
echo ALLDONE
