#!/bin/bash
# real-crypto mode: GPU tests, then the crypto bench line and the cfg3 line (stdout must be one JSON line)
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
export PYTHONUNBUFFERED=1
timeout -k 10 600 python -u -m pytest tests/test_gpu_crypto.py tests/test_gpu_comm.py -x -v -m gpu --timeout 200 --timeout-method thread > $O/crypto_tests.log 2>&1
rc=$?
tail -3 $O/crypto_tests.log
[ $rc -eq 0 ] || { grep -E "FAILED|Error" $O/crypto_tests.log | head -20; exit $rc; }
timeout -k 10 400 python bench.py --workload crypto --steps 3 --warmup 1 --full > $O/bench_crypto.json 2> $O/bench_crypto.err || exit $?
cat $O/bench_crypto.json
timeout -k 10 300 python bench.py --steps 20 --warmup 3 --full --no-cpu > $O/bench.json 2> $O/bench.err || exit $?
python -c "import json; d=json.load(open('$O/bench.json')); print(round(d['value']/1e6,1), 'M instance-rounds/s', d['config']['stats_allreduce'])"
