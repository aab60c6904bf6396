# Same-box A/B of two libmiba builds (abl/libmiba_<name>.so) on C4: bench value + per-kernel ms,
# alternating builds to cancel clock drift. usage: bash tools/ab_lib.sh "old new ..." [rounds] [config]
# Logs go to $MIBA_AB_OUT (default ab_out/).
set -o pipefail
cd $GRAFT_REPO_ROOT
rounds=${2:-3}; cfg=${3:-C4}
export MIBA_AB_OUT=${MIBA_AB_OUT:-ab_out}
mkdir -p $MIBA_AB_OUT
for r in $(seq 1 $rounds); do
  for name in $1; do
    log=$MIBA_AB_OUT/ab_${name}_$r.log
    MIBA_LIB_PATH=$PWD/abl/libmiba_$name.so timeout -k 10 200 python bench.py --full --no-cpu-baseline --config $cfg > $log 2>&1 || { echo "FAIL $name"; tail -5 $log; exit 1; }
    python - "$name" "$log" <<'PY'
import json,sys
d=json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
k=d.get('kernel_ms_per_step') or {}
print(f"{sys.argv[1]:8s} {d['value']:9.1f} {d['ms_per_step']*1e3:7.1f} us/it bcr_avg={d.get('roofline',{}).get('avg_launch_ms',0)*1e3:.1f} |", " ".join(f"{n}={v*1e3:.1f}" for n,v in k.items()))
PY
  done
done
