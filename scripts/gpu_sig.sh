#!/bin/bash
# secp256k1 measurement pass (through gpurun): parity tests, the multiply-add peak, throughput, and a
# rocprofv3 kernel trace of the throughput run (summary in $O/sigprof).
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O/sigprof
export PYTHONUNBUFFERED=1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 300 python -u -m pytest tests/test_gpu_sig.py -x -q --timeout 240 --timeout-method thread > $O/sig_tests.log 2>&1 || { tail -30 $O/sig_tests.log; exit 1; }
tail -2 $O/sig_tests.log
timeout -k 10 60 consensus-rs_amd/build/mad_peak > $O/mad_peak.json && cat $O/mad_peak.json && \
timeout -k 10 200 python scripts/sig_bench.py --n 262144 --reps 3 > $O/sig_bench.json && cat $O/sig_bench.json && \
timeout -k 10 200 python bench.py --workload sig --steps 10 --warmup 2 --full > $O/bench_sig.json && cat $O/bench_sig.json && \
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/sigprof -o run --output-format csv -- python3 bench.py --workload sig --steps 10 --warmup 2 --no-cpu > $O/sigprof/bench.json 2> $O/sigprof/err.txt
rc=$?
cat $O/sigprof/run_kernel_stats.csv 2>/dev/null | cut -c1-150
exit $rc
