#!/bin/bash
# round-6 experiment 1: cfg 2 with the stash in chunks small enough for the Infinity Cache
# usage: bash tools/r6_chunk_experiment.sh <output directory>
OUT=${1:?usage: bash tools/r6_chunk_experiment.sh <output directory>}
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
python3 bench.py --full --steps 50 --warmup 20 > "$OUT/chunk_base.json" 2> "$OUT/chunk_base.err"
for mb in 48 96 144 192 240 400; do
  NF_AFFINE_STASH_MAX_MB=$mb python3 bench.py --full --steps 50 --warmup 20 > "$OUT/chunk_$mb.json" 2> "$OUT/chunk_$mb.err"
done
python3 bench.py --full --steps 50 --warmup 20 > "$OUT/chunk_base2.json" 2> "$OUT/chunk_base2.err"
python3 - "$OUT" <<'PY'
import json,glob,os,sys
for f in sorted(glob.glob(os.path.join(sys.argv[1], 'chunk_*.json'))):
    for l in open(f):
        l=l.strip()
        if l.startswith('{'):
            d=json.loads(l)
            print(f, d['ms_per_step'], d.get('ms_per_step_sustained_clock'), {k:(v['avg_ms'],v['launches_per_step']) for k,v in d.get('kernels',{}).items()})
PY
