#!/bin/bash
# same-box A/B of two trees: tools/ab_bench.sh <other tree> [rounds] [out dir] -> <out dir>/ab_<k>_{base,new}.json
# (default out dir: bench_out; --full for the per-family roofline, no CPU leg)
other=$1; rounds=${2:-2}; out=${3:-bench_out}
mkdir -p $out
for k in $(seq 1 $rounds); do
  (cd $other && python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline) > $out/ab_${k}_base.json 2> $out/ab_${k}_base.err
  python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline > $out/ab_${k}_new.json 2> $out/ab_${k}_new.err
done
python - "$out" <<'P'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + '/ab_*_*.json')):
    try:
        d=json.load(open(f)); fam=d['roofline']['families']
        print(f, d['value'], d['ms_per_step'], {k.split(' ')[0][:22]:v['ms_per_step'] for k,v in list(fam.items())[:9]})
    except Exception as e: print(f,'ERR',e)
P
