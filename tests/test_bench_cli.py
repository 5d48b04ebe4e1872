"""bench.py's command line: a plain run measures the headline only, --dump-outputs writes what the last timed step computed,
--full carries the other legs (roofline, PMC passes, comparison legs, CPU baseline)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def test_bench_help_lists_full_and_dump_outputs():
    p = subprocess.run([sys.executable, BENCH, '--help'], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert '--full' in p.stdout and '--dump-outputs' in p.stdout


@pytest.mark.gpu
def test_plain_bench_times_the_given_steps_and_dumps_its_outputs(tmp_path):
    out = tmp_path / 'dump'
    cmd = [sys.executable, BENCH, '--gpus', '1', '--steps', '3', '--warmup', '2', '--batch', '2', '--dim', '32',
           '--settle', '10', '--dump-outputs', str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in res, k
    assert res['steps'] == 3 and res['warmup'] == 2 and res['ms_per_step'] > 0 and res['value'] > 0
    # the plain run stops after the headline: nothing of --full
    assert res['roofline'] is None and res['cpu_baseline'] is None and res['other_legs'] is None
    names = sorted(os.listdir(out))
    assert names == ['level_losses.npy', 'loss.npy', 'model_state.npy'], names
    total = 0
    for n in names:
        a = np.load(out / n)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(out / 'model_state.npy').size > 643735          # every parameter + the BatchNorm buffers
