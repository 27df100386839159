# GPU-box check: parity tests, then a bench line.  usage: TAG=r2_ BENCH_ARGS="..." bash scripts/gpu_check.sh
set -o pipefail
cd $GRAFT_REPO_ROOT
TAG=${TAG:-r1_}
O=${OUT:-out}  # where the logs go
mkdir -p $O
(nproc; rocm-smi --showproductname 2>&1 | head -20) > $O/${TAG}info.txt || true
timeout -k 10 400 python -m pytest tests -m gpu -x -q > $O/${TAG}pytest.log 2>&1
rc=$?; echo "pytest rc=$rc" >> $O/${TAG}pytest.log; tail -5 $O/${TAG}pytest.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python bench.py --full ${BENCH_ARGS} > $O/${TAG}bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -2 $O/${TAG}bench.log
exit $rc
