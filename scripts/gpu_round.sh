# Round evidence: GPU parity tests, the default bench line (with the CPU baseline), then per config a
# rocprofv3 kernel trace + stats and FETCH_SIZE / WRITE_SIZE PMC passes.  usage: TAG=r01f_ bash scripts/gpu_round.sh
set -o pipefail
R=$GRAFT_REPO_ROOT
TAG=${TAG:-r01f_}
O=${OUT:-out}  # where the logs go
mkdir -p $O
cd $R
timeout -k 10 400 python -m pytest tests -m gpu -q > $O/${TAG}pytest.log 2>&1 || { tail -30 $O/${TAG}pytest.log; exit 1; }
tail -1 $O/${TAG}pytest.log
timeout -k 10 400 python bench.py --full > $O/${TAG}bench.log 2>&1 || { tail -5 $O/${TAG}bench.log; exit 1; }
tail -1 $O/${TAG}bench.log
for c in ${CONFIGS:-jumpy-1080p cornell-800 cow-1080p monument-4k jumpy-400}; do
  TAG=${TAG}${c}_ ARGS="--config $c --steps 2 --warmup 1 --no-cpu-baseline" PMC_ARGS="--config $c" bash scripts/gpu_profile.sh > /dev/null || exit $?
  echo "profiled $c"
done
