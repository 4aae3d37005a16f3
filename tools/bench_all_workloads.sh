# Dev helper (GPU box): one bench line per named workload (BASELINE.md §2's table).
OUT=${OUT:-bench_runs}   # where the JSON lines go
mkdir -p "$OUT"
for w in c1_1k_128x128 lego_like_300k_800x800 scannetpp_like_fisheye_300k_1752x1168 garden_like_5M_1297x840; do
  python bench.py --full --workload $w > "$OUT/wl_$w.json" 2> "$OUT/wl_$w.err"; echo "$w rc $?"
done
python bench.py --full --force-exchange --no-sensitivity --no-drop-in --no-cpu-baseline > "$OUT/wl_force_exchange.json" 2> "$OUT/wl_force_exchange.err"; echo "force-exchange rc $?"
