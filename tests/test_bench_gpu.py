"""bench.py's plain run: the headline only (no measurement beyond the timed steps), `--steps` timed steps, and
`--dump-outputs DIR` writing the last timed step's outputs, the epoch means and the updated parameters as DIR/<name>.npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_times_the_steps_only_and_dumps_the_last_step(tmp_path):
    out = tmp_path / 'outputs'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', 'C0', '--batch', '8', '--steps', '3',
           '--warmup', '1', '--dump-outputs', str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'VQCPC_FORCE_DIST')}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in line, key
    assert line['steps'] == 3 and line['n_gpus'] == 1 and line['unit'] == 'windows/s' and line['dtype'] == 'f32'
    assert abs(line['value'] - 8 * 3 / (line['ms_per_step'] * 3e-3)) < 0.01 * line['value']
    # everything beyond the headline is --full only
    for key in ('roofline', 'cpu_baseline', 'train_step_only', 'clock', 'allreduce', 'n1_same_node'):
        assert line[key] is None, key
    for key in ('secondary', 'c1_long', 'extra_six_product_gradients', 'extra_six_product_forward'):
        assert key not in line, key

    files = sorted(os.listdir(out))
    for name in ('params.npy', 'step_loss.npy', 'step_idx_left.npy', 'epoch_loss.npy'):
        assert name in files, files
    total = 0
    for f in files:
        a = np.load(out / f, allow_pickle=False)
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        assert np.all(np.isfinite(a)), f
        total += os.path.getsize(out / f)
    assert total <= 64e6
    assert np.load(out / 'params.npy').size == line['config']['params']
    assert abs(float(np.load(out / 'epoch_loss.npy')) - line['final_loss']) < 1e-4
