# The measurements of a round on its final build (GPU box): the seven rocprofv3 passes of tools/profile.sh + the bench variants.
#   usage: OUT=<dir> bash tools/measure.sh <tag>      -> $OUT/<tag>_*  (OUT defaults to out/)
# Every bench line but the driver's runs with --full (per-kernel figures and roofline; the default line also the secondary measurements
# and the CPU baseline); the driver line is the plain run the headline figure comes from.
TAG=${1:-r06}
OUT=${OUT:-out}
set -u
mkdir -p "$OUT"
bash tools/profile.sh ${TAG} > "$OUT/${TAG}_profile.log" 2>&1
python bench.py --full > "$OUT/${TAG}_bench_default.json" 2> "$OUT/${TAG}_bench_default.err"
python bench.py --steps 20 --warmup 5 > "$OUT/${TAG}_bench_driver.json" 2>/dev/null
V="--full --no-cpu-baseline --no-single-stream --easy-noise 0"
python bench.py $V --streams 1 --batch 1024 > "$OUT/${TAG}_bench_slice1.json" 2>/dev/null
python bench.py $V --batch 32768 > "$OUT/${TAG}_bench_b32768.json" 2>/dev/null
python bench.py $V --batch 8192 > "$OUT/${TAG}_bench_b8192.json" 2>/dev/null
python bench.py $V --workload atlas20_freefall > "$OUT/${TAG}_bench_freefall.json" 2>/dev/null
python bench.py $V --workload atlas33_contact --batch 8192 > "$OUT/${TAG}_bench_atlas33.json" 2>/dev/null
python bench.py $V --workload atlas33_contact --rollout 64 --batch 8192 > "$OUT/${TAG}_bench_atlas33_rollout.json" 2>/dev/null
python bench.py $V --workload atlas33_contact --rollout 64 --batch 8192 --graph > "$OUT/${TAG}_bench_atlas33_rollout_graph.json" 2>/dev/null
python bench.py $V --workload atlas33_contact --rollout 64 --batch 8192 --checkpoint-every 16 > "$OUT/${TAG}_bench_atlas33_rollout_checkpoint16.json" 2>/dev/null
python bench.py $V --rollout 64 > "$OUT/${TAG}_bench_atlas20_rollout.json" 2>/dev/null
python bench.py $V --rollout 64 --graph > "$OUT/${TAG}_bench_atlas20_rollout_graph.json" 2>/dev/null
python bench.py $V --max-contacts 16 > "$OUT/${TAG}_bench_48rows.json" 2>/dev/null
python bench.py $V --max-contacts 24 --steps 8 --warmup 2 > "$OUT/${TAG}_bench_general.json" 2>/dev/null
NBL_FUSED_DETECT=0 python bench.py $V > "$OUT/${TAG}_bench_unfused_detect.json" 2>/dev/null
for f in "$OUT"/${TAG}_bench_*.json; do echo $f; tail -1 $f | cut -c1-260; done
