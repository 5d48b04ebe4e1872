#!/bin/bash
# what the driver runs at round end, on the working tree: smoke, the bench command line of the contract, the GPU suite
TAG=$1; OUT=${OUT:-out}; mkdir -p $OUT   # OUT: output folder, relative to the repository root
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1; echo "smoke rc $?"; tail -1 $OUT/${TAG}_smoke.log
T0=$(date +%s)
timeout -k 10 900 python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/${TAG}_driver_cmd.json 2> $OUT/${TAG}_driver_cmd.err
echo "driver bench rc $? in $(( $(date +%s) - T0 )) s"
python -c "import json; d=json.loads(open('$OUT/${TAG}_driver_cmd.json').read().strip().splitlines()[-1]); print(d['metric'], d['value'], d['unit'], d['ms_per_step'], d['dtype'])"
timeout -k 10 1500 python -m pytest tests -m gpu -q -x > $OUT/${TAG}_pytest_gpu.log 2>&1; echo "pytest rc $?"; tail -2 $OUT/${TAG}_pytest_gpu.log
