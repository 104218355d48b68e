#!/bin/bash
# where to switch k_surfel_pass from quarter-tile units to whole tiles + resident grid (tiles of the slot estimate).  usage: tools/r3_thr.sh <tag>
: "${OUT_DIR:?set OUT_DIR to the folder the results go to}"
tag=${1:-r3thr}
for st in 100 200; do for thr in 4096 8192 16384 1000000; do
  SM_PASS_PERSIST_TILES=$thr timeout -k 10 300 python bench.py --full --steps $st --warmup 10 --only-headline --no-cpu-baseline > $OUT_DIR/${tag}_${st}_$thr.json 2>> $OUT_DIR/${tag}.err || exit 1
  python - $OUT_DIR/${tag}_${st}_$thr.json $thr <<PY
import json,sys
d=json.load(open(sys.argv[1])); k=d['kernels']
print("threshold", sys.argv[2], "steps", d["steps"], "value", round(d["value"]), round(d["ms_per_step"]*1e3,2), "us", {n:round(v['ms']*1e3,1) for n,v in k.items() if n in('k_assoc_prep','k_surfel_pass')})
PY
done; done
