# quick knob sweep: bench one config under several env settings (after the parity tests pass)
set -o pipefail
cd $GRAFT_REPO_ROOT
TAG=${TAG:-sw_}
O=${OUT:-out}  # where the logs go
mkdir -p $O
timeout -k 10 300 python -m pytest tests -m gpu -x -q > $O/${TAG}pytest.log 2>&1 || { tail -20 $O/${TAG}pytest.log; exit 1; }
tail -1 $O/${TAG}pytest.log
for kv in $SWEEP; do
  env $kv timeout -k 10 200 python bench.py --steps 3 --warmup 1 --full --no-cpu-baseline $BENCH_ARGS > $O/${TAG}$kv.log 2>&1 || exit $?
  echo "$kv $(grep -o '"value": [0-9.]*' $O/${TAG}$kv.log) $(grep -o '"simd_util_rank0": {[^}]*}' $O/${TAG}$kv.log) $(grep -o '"phase_share_rank0": {[^}]*}' $O/${TAG}$kv.log)"
done
