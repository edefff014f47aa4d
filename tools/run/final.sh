set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT/prof
rm -rf $OUT/prof/*
timeout -k 10 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"; python tools/show_bench.py $OUT/bench.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r01d -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-train --no-pooled > $OUT/prof_bench.json 2> $OUT/prof.err; echo "prof rc=$?"
python tools/show_bench.py $OUT/prof_bench.json
