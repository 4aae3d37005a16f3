# Dev helper (GPU box): bench legs with / without an environment switch, interleaved.  usage: bash tools/ab_env.sh VAR TAG workload...
VAR=$1; TAG=$2; shift 2
OUT=${OUT:-bench_runs}   # where the JSON lines go
mkdir -p "$OUT"
for i in 1 2; do
  for v in off on; do
    for w in "$@"; do
      if [ $v = on ]; then export $VAR=1; else unset $VAR; fi
      python bench.py --full --workload $w --no-sensitivity --no-drop-in --no-cpu-baseline > "$OUT/ab_${TAG}_${w}_${v}_${i}.json" 2> "$OUT/ab_${TAG}.err"
    done
  done
done
