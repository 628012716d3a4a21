set -o pipefail
export OUT=${XPG_OUT_DIR:-bench_out}  # logs, traces and counter files of these runs
mkdir -p "$OUT"
for r in 1 2; do
timeout -k 10 200 python bench.py --full --sections headline --no-cpu-baseline > $OUT/hb_base_$r.log 2>&1 || exit $?
XPG_BENCH_FIT_DEPTH=1 timeout -k 10 200 python bench.py --full --sections headline --no-cpu-baseline --repeats 2 --steps 10 > $OUT/hb_r2l1_$r.log 2>&1 || exit $?
timeout -k 10 200 python bench.py --full --sections headline --no-cpu-baseline --repeats 2 --steps 10 > $OUT/hb_r2l2_$r.log 2>&1 || exit $?
XPG_BENCH_FIT_DEPTH=1 timeout -k 10 200 python bench.py --full --sections headline --no-cpu-baseline --repeats 4 --steps 8 > $OUT/hb_r4l1_$r.log 2>&1 || exit $?
done
