#!/bin/bash
# Round-end evidence on one box: full GPU suite, smoke, full bench line, rocprofv3 kernel stats of
# the bench (each step under its own limit; stop at the first fault / abort / time-out)
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
export OUT=${XPG_OUT_DIR:-bench_out}  # logs, traces and counter files of these runs
mkdir -p "$OUT"
export PYTHONUNBUFFERED=1
timeout -k 10 900 python -u -m pytest tests -m gpu -q -rf --timeout 300 --timeout-method thread > $OUT/final_tests.log 2>&1; rc=$?
echo "tests rc=$rc"; tail -3 $OUT/final_tests.log
case $rc in 0|1) ;; *) exit $rc ;; esac
timeout -k 10 300 python __graft_entry__.py smoke > $OUT/final_smoke.log 2>&1 || exit $?
timeout -k 10 600 python bench.py --full > $OUT/final_bench.log 2>&1 || exit $?
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final_prof -o run -- python3 bench.py --full --steps 6 --warmup 2 --no-cpu-baseline > $OUT/final_prof.log 2>&1 || exit $?
echo done
