# every config under each RTW_OCC setting (after the parity tests pass)
set -o pipefail
export RTW_TUNING=1  # the library reads tuning knobs only with the gate open
cd $GRAFT_REPO_ROOT
TAG=${TAG:-oc_}
O=${OUT:-out}  # where the logs go
mkdir -p $O
timeout -k 10 300 python -m pytest tests -m gpu -x -q > $O/${TAG}pytest.log 2>&1 || { tail -20 $O/${TAG}pytest.log; exit 1; }
tail -1 $O/${TAG}pytest.log
for o in ${OCCS:-4 5}; do
  for c in ${CONFIGS:-jumpy-1080p cornell-800 cow-1080p monument-4k}; do
    RTW_OCC=$o timeout -k 10 300 python bench.py --config $c --steps 2 --warmup 1 --full --no-cpu-baseline > $O/${TAG}$o$c.log 2>&1 || { tail -5 $O/${TAG}$o$c.log; exit 1; }
    echo "occ$o $c $(grep -o '"value": [0-9.]*' $O/${TAG}$o$c.log) $(grep -o '"phase_share_rank0": {[^}]*}' $O/${TAG}$o$c.log)"
  done
done
