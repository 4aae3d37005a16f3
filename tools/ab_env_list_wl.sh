# Dev helper (GPU box): one bench workload under a list of environment settings.  usage: bash tools/ab_env_list_wl.sh TAG WORKLOAD "A=1" "X=" ...
tag=$1; wl=$2; shift; shift
OUT=${OUT:-bench_runs}   # where the JSON lines go
mkdir -p "$OUT"
k=0
for envs in "$@"; do
  k=$((k+1))
  env $envs python bench.py --full --workload $wl --no-sensitivity --no-drop-in --no-cpu-baseline > "$OUT/env_${tag}_${k}.json" 2> "$OUT/env_${tag}.err"
done
