set -o pipefail
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 1000 python -m pytest tests -q -m gpu -x > $OUT/t1.log 2>&1; rc=$?; tail -5 $OUT/t1.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; rc=$?; tail -4 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
OUT=$OUT bash tools/run/final.sh
