#!/bin/bash
# compaction period sweep on the two-launch code.  usage: tools/r3_period.sh <tag>
: "${OUT_DIR:?set OUT_DIR to the folder the results go to}"
tag=${1:-r3per}
for st in 100 200; do for p in 12 16 24 32 48; do
  timeout -k 10 300 python bench.py --full --steps $st --warmup 10 --compact-period $p --only-headline --no-cpu-baseline > $OUT_DIR/${tag}_${st}_$p.json 2>> $OUT_DIR/${tag}.err || exit 1
  python - $OUT_DIR/${tag}_${st}_$p.json $p <<PY
import json,sys
d=json.load(open(sys.argv[1])); k=d['kernels']
print("period", sys.argv[2], "steps", d["steps"], "value", round(d["value"]), round(d["ms_per_step"]*1e3,2), "us", {n:(round(v['ms']*1e3,1), v['launches']) for n,v in k.items() if n in('k_assoc_prep','k_surfel_pass','k_compact','k_conflict')})
PY
done; done
