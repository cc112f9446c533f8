#!/bin/bash
# wire-codec measurement pass (through gpurun): parity tests, bench line, rocprofv3 kernel trace.
set -o pipefail
export O=${OUT_DIR:-bench_out}
mkdir -p $O/wireprof
export PYTHONUNBUFFERED=1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 300 python -u -m pytest tests/test_gpu_wire.py -x -q --timeout 240 --timeout-method thread > $O/wire_tests.log 2>&1 || { tail -30 $O/wire_tests.log; exit 1; }
tail -2 $O/wire_tests.log
timeout -k 10 200 python bench.py --workload wire --steps 10 --warmup 2 --full > $O/bench_wire.json && cat $O/bench_wire.json && \
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/wireprof -o run --output-format csv -- python3 bench.py --workload wire --steps 10 --warmup 2 --no-cpu > $O/wireprof/bench.json 2> $O/wireprof/err.txt
rc=$?
python3 - <<'PY'
import csv, os
for r in csv.DictReader(open(os.environ["O"] + "/wireprof/run_kernel_stats.csv")):
    print(r["Name"][:60], r["Calls"], round(float(r["AverageNs"]) / 1e3, 1), "us", r["Percentage"])
PY
exit $rc
