#!/bin/bash
# quarter-tile units in k_surfel_pass: parity subset under both forms, then A/B bench lines.  usage: tools/r3_split.sh <tag>
: "${OUT_DIR:?set OUT_DIR to the folder the results go to}"
tag=${1:-r3split}
timeout -k 10 600 python -m pytest tests/test_kat.py tests/test_gpu_parity.py tests/test_deferred_compaction.py tests/test_fuzz_gpu.py tests/test_shard_stream.py -m gpu -x -q > $OUT_DIR/${tag}_pytest.log 2>&1; rc=$?
tail -n 3 $OUT_DIR/${tag}_pytest.log; [ $rc -ne 0 ] && exit 1
SM_PASS_SPLIT=4 timeout -k 10 600 python -m pytest tests/test_configs_full_size.py tests/test_rig.py -m gpu -x -q > $OUT_DIR/${tag}_pytest4.log 2>&1; rc=$?
tail -n 3 $OUT_DIR/${tag}_pytest4.log; [ $rc -ne 0 ] && exit 1
SM_PASS_SPLIT=1 timeout -k 10 600 python -m pytest tests/test_kat.py tests/test_deferred_compaction.py tests/test_fuzz_gpu.py -m gpu -x -q > $OUT_DIR/${tag}_pytest1.log 2>&1; rc=$?
tail -n 3 $OUT_DIR/${tag}_pytest1.log; [ $rc -ne 0 ] && exit 1
run() { # name, env..., -- bench args
  name=$1; shift
  env "$@" timeout -k 10 300 python bench.py --full $BARGS --only-headline --no-cpu-baseline > $OUT_DIR/${tag}_$name.json 2>> $OUT_DIR/${tag}_bench.err || return 1
  python - $OUT_DIR/${tag}_$name.json $name <<PY
import json,sys
d=json.load(open(sys.argv[1])); k=d['kernels']
print(sys.argv[2], "value", round(d["value"]), round(d["ms_per_step"]*1e3,2), "us", {n:round(v['ms']*1e3,1) for n,v in k.items() if n in('k_assoc_prep','k_surfel_pass','k_pass_fixup')})
PY
}
for cfg in "20 5" "100 10"; do set -- $cfg; BARGS="--steps $1 --warmup $2"
  run s1_$1 SM_PASS_SPLIT=1 && run s4_$1 SM_PASS_SPLIT=4 || exit 1
done
BARGS="--workload hd20m --steps 40 --warmup 5"
run hd_s1 SM_PASS_SPLIT=1 && run hd_s4 SM_PASS_SPLIT=4
