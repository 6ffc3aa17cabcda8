# Evidence of one round:  bash tools/collect_profiles.sh <tag>   -> ${PROFILE_RUNS:-profile_runs}/<tag>/
#   kernel stats (rocprofv3 --kernel-trace --stats) of the default bench, PMC HBM traffic passes, the default bench line,
#   and one line per BASELINE config.
TAG=${1:-final}
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && D=${PROFILE_RUNS:-profile_runs}/$TAG && mkdir -p $D
rocprofv3 --kernel-trace --stats --output-format csv -d $D/stats -- python3 bench.py --steps 10 --warmup 3 --no-cpu-baseline > $D/bench_under_rocprof.json 2> $D/stats.err
bash tools/pmc_traffic.sh $TAG/traffic > /dev/null 2>&1
python3 tools/make_traffic_json.py $D/traffic $D/traffic.json > $D/traffic.txt
python3 bench.py --full > $D/bench.json 2> $D/bench.err
: > $D/configs.jsonl
for w in cora pubmed arxiv; do
  python3 bench.py --workload $w --steps 300 --warmup 30 --no-cpu-baseline --graph --full >> $D/configs.jsonl 2>/dev/null
  python3 bench.py --workload $w --steps 300 --warmup 30 --no-cpu-baseline --full >> $D/configs.jsonl 2>/dev/null
done
python3 bench.py --workload products --dtype bf16 --no-cpu-baseline --full >> $D/configs.jsonl 2>/dev/null
python3 bench.py --workload pl10m --dtype bf16 --steps 5 --warmup 2 --no-cpu-baseline --full >> $D/configs.jsonl 2>/dev/null
ls $D
