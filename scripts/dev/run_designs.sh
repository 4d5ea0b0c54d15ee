# the reference's own benchmark designs (benchmark/generate_matrices.py) + cfg1 through bench.py --full -> OUTDIR
# usage: bash scripts/dev/run_designs.sh [OUTDIR]   (default bench_out/designs)
O=${1:-bench_out/designs}
mkdir -p $O
for w in dense one_cat two_cat dense_cat dense_smallcat sparse sparse_narrow sparse_wide cfg1; do
  python bench.py --full --workload $w --steps 10 --warmup 3 --no-traffic > $O/bench_$w.json 2> $O/$w.err || echo "FAILED $w"
  python -c "
import json
d=json.load(open('$O/bench_$w.json')); print('$w', d['ms_per_step'], d['roofline']['kernel'], d['roofline']['frac'], (d.get('matvec') or {}).get('ms'), (d.get('transpose_matvec') or {}).get('ms'))"
done
