# Dev helper (GPU box): the bench's headline leg under a list of environment settings, in the order given, twice around.
# usage: bash tools/ab_env_list.sh TAG "A=1 B=2" "A=0" ...   (an empty string = no setting)
tag=$1; shift
OUT=${OUT:-bench_runs}   # where the JSON lines go
mkdir -p "$OUT"
for i in 1 2; do
  k=0
  for envs in "$@"; do
    k=$((k+1))
    env $envs python bench.py --full --no-sensitivity --no-drop-in --no-cpu-baseline > "$OUT/env_${tag}_${k}_${i}.json" 2> "$OUT/env_${tag}.err"
  done
done
