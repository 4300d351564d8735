# full round check on the GPU box: -m gpu tests, smoke, bench --full -> <out-dir>/
# usage: tools/run_full.sh <out-dir>   (run from anywhere; the tree is the one this script lies in)
# Every step has a time limit of its own; the first step that fails, aborts, faults or times out ends the script, so
# nothing more is started on a card that may be in a bad state.
set -u
OUT=$(mkdir -p "$1" && cd "$1" && pwd)
cd "$(dirname "$0")/.."
step() {   # step <name> <timeout-s> <cmd...>: stdout / stderr -> $OUT/<name>.log, exit status and wall clock reported
  local name=$1 lim=$2; shift 2
  local t0=$(date +%s)
  timeout -k 10 "$lim" "$@" > "$OUT/$name.log" 2>&1
  local rc=$?
  echo "$name rc=$rc wall_s=$(( $(date +%s) - t0 ))"
  if [ $rc -ne 0 ]; then tail -20 "$OUT/$name.log"; exit $rc; fi
}
step pytest 1800 python -m pytest tests -m gpu -x -q
tail -2 $OUT/pytest.log
step smoke 600 python -c "import __graft_entry__ as g; g.smoke()"
tail -2 $OUT/smoke.log
step bench 900 sh -c 'exec python bench.py --full > "$1/bench.json"' _ "$OUT"
python - "$OUT/bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
for k in ('value','ms_per_step','rtf','step_ms'): print(k, d.get(k))
for k in ("audio_only_call","dense_worst_case","moving_f0","single_stream","single_stream_graph","single_stream_native","native_group_call","whole_file"): print(k, {kk:vv for kk,vv in d.get(k,{}).items() if kk!='workload'})
print('roofline', {k:d['roofline'][k] for k in ('frac','ms_per_launch')})
print('roofline_step', d['roofline_step'])
c=d['cpu_baseline']; print('cpu', c['value'], c['cores'], c['kind'], c['sample'][:160])
print('midi_like', {kk:vv for kk,vv in d.get('midi_like',{}).items() if kk!='workload'})
ch=d['roofline'].get('three_operator_chain'); print('chain', ch and ch['ms'], ch and ch['frac_of_measured_write'])
PY
