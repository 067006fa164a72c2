# round-end measurement: rocprofv3 trace + PMC passes (tools/profile_round.sh), then the full bench lines of every
# config; each GPU step under its own limit, stopping at the first failure
cd "$(dirname "$0")/.."; OUT="${OUT:-bench_out}"; mkdir -p "$OUT"
bash tools/profile_round.sh || exit $?
for c in ${CONFIGS:-c1 c2 c3 c4}; do
  timeout -k 10 300 python bench.py --full --config $c ${BENCH_ARGS} > "$OUT/eor_bench_$c.log" 2>&1; rc=$?
  echo "bench $c rc=$rc"; tail -c 400 "$OUT/eor_bench_$c.log"; echo; [ $rc -eq 0 ] || exit $rc
done
