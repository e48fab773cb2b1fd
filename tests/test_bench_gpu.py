"""GPU: a plain `bench.py` run times the headline step and nothing else, and `--dump-outputs` writes what its last timed step
computed (tests/test_bench_outputs_cpu.py checks the files themselves on the specification library)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_line_and_dumps_the_last_step(tmp_path):
    out = tmp_path / 'outputs'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--dump-outputs', str(out)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d['metric'] == 'frustums/sec fwd+bwd' and d['unit'] == 'frustums/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32' and d['steps'] == 3 and d['warmup'] == 1
    assert d['ms_per_step'] > 0 and abs(d['value'] - 32 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
    assert d['roofline'] is None and d['cpu_baseline'] is None and d['other_configs'] is None
    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {'loss', 'logits', 'weights', 'grads', 'moving_stats'} <= set(files)
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files['logits'].shape == (32, 1024, 2) and np.isfinite(files['weights']).all()
    assert float(files['loss'].reshape(-1)[0]) == np.float32(d['config']['final_loss'])
