# GPU tests, the mode-hypothesis bench line and the --extra lines (full records: rooflines included).
# OUT=<folder for the logs> TAG=<prefix> bash tools/gpu_modes.sh
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${OUT:?set OUT to the folder for the logs}
T=${TAG:-m1}
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/$T.pytest.log 2>&1 || { echo "pytest rc=$?"; tail -30 $O/$T.pytest.log; exit 1; }
tail -3 $O/$T.pytest.log
timeout -k 10 200 python bench.py --full --config modes16_b16384 --steps 20 --warmup 3 --no-cpu-baseline > $O/$T.bench_modes.log 2>&1 || { echo bench_modes rc=$?; tail $O/$T.bench_modes.log; exit 1; }
tail -1 $O/$T.bench_modes.log
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 --extra --no-cpu-baseline > $O/$T.bench_extra.log 2>&1 || { echo bench_extra rc=$?; tail $O/$T.bench_extra.log; exit 1; }
tail -1 $O/$T.bench_extra.log
