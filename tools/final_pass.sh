#!/bin/bash
# usage (GPU box, repo root): tools/final_pass.sh <outdir>  -> smoke, GPU tests, the --full bench lines, kernel stats and PMC traffic
set -e
export TMPDIR=/tmp
ROOT=$(pwd)
O=${1:?usage: tools/final_pass.sh <outdir>}
mkdir -p $O
python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; tail -1 $O/smoke.log
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1; tail -1 $O/pytest_gpu.log
timeout -k 10 400 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
for w in tiny4096 blox4096 mazes4096 mazes8192; do timeout -k 10 300 python bench.py --full --workload $w --no-ppo > $O/bench_$w.json 2>/dev/null; done
timeout -k 10 300 python bench.py --full --obs bfloat16 --no-ppo > $O/bench_small_bfloat16.json 2>/dev/null
timeout -k 10 300 python bench.py --full --obs uint8 --no-ppo > $O/bench_small_uint8.json 2>/dev/null
timeout -k 10 300 python bench.py --full --envs 65536 --no-ppo > $O/bench_small65536.json 2>/dev/null
timeout -k 10 300 python bench.py --full --workload blox4096 --envs 16384 --no-ppo > $O/bench_blox16384.json 2>/dev/null
cd /tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_final -o fin -- python3 $ROOT/bench.py --full --steps 300 --warmup 50 --no-cpu-baseline --no-ppo --no-unidirectional > /tmp/prof_final.log 2>&1
cd $ROOT
cp $(find /tmp/prof_final -name "*kernel_stats.csv" | head -1) $O/kernel_stats_small16384_f32.csv
bash tools/pmc_pass.sh small16384 float32 fin > $O/pmc.log 2>&1 || echo "pmc pass failed"
# the traffic of this pass alone, from the counter runs pmc_pass.sh left under /tmp
python tools/pmc_traffic.py /tmp/pmc_fin_FETCH_SIZE /tmp/pmc_fin_WRITE_SIZE small16384:float32 $O/traffic_small16384_f32.json 2>/dev/null || true
python tools/pmc_traffic.py /tmp/pmc_fin_FETCH_SIZE /tmp/pmc_fin_WRITE_SIZE small16384:emit_uint8 $O/traffic_small16384_f32.json pmx_emit_team 2>/dev/null || true
echo done
