cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for m in full_adam dense_adam adagrad sgd; do
  python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --update-method $m > "$OUT/bench_$m.json" 2> "$OUT/bench_$m.err"
done
python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --uniform-words > "$OUT/bench_uniform.json" 2>&1
python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --host-batches > "$OUT/bench_hostbatches.json" 2>&1
python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --read-cost-every 1 > "$OUT/bench_readcost.json" 2>&1
python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --config large_tables > "$OUT/bench_large.json" 2>&1
python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --config lse_small > "$OUT/bench_small.json" 2>&1
OUT="$OUT" python - <<'PY'
import json,glob,os
for f in sorted(glob.glob(os.path.join(os.environ['OUT'], 'bench_*.json'))):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1])
        print(f.split('/')[-1], d['value'], d['ms_per_step'], d['config']['update_method'], d['roofline']['kernel'], d['roofline']['frac'])
    except Exception as e:
        print(f, 'ERR', e, open(f).read()[-300:])
PY
