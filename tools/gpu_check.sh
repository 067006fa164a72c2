cd "$(dirname "$0")/.."; OUT="${OUT:-bench_out}"; mkdir -p "$OUT"
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/eor_tests.log" 2>&1; rc=$?; echo "tests rc=$rc"; tail -3 "$OUT/eor_tests.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python tools/session_bench.py > "$OUT/sess_u.log" 2>&1 || exit $?; tail -1 "$OUT/sess_u.log"
SB_ZIPF=1.2 timeout -k 10 200 python tools/session_bench.py > "$OUT/sess_z.log" 2>&1 || exit $?; tail -1 "$OUT/sess_z.log"
timeout -k 10 300 python bench.py --full --cpu-sample 0 --decode-steps 0 --h2d-steps 0 > "$OUT/drain_c1.log" 2>&1 || exit $?; tail -c 420 "$OUT/drain_c1.log"
