"""bench.py --dump-outputs on the host: dtypes, names and the 64 MB budget (larger arrays become a fixed seeded sample)."""
import importlib.util
import os

import numpy as np
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location('vqcpc_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    env = dict(os.environ)
    try:
        spec.loader.exec_module(mod)
    finally:                                                # bench.py sets process-wide defaults for its own runs
        os.environ.clear()
        os.environ.update(env)
    return mod


def test_dump_outputs_names_dtypes_and_budget(tmp_path):
    bench = _bench()
    step = dict(loss=torch.tensor(1.5), idx_left=torch.arange(12).reshape(6, 2), accuracy=torch.rand(4, dtype=torch.float64))
    means = dict(loss=1.25, accuracy=[0.5, 0.25], num_codewords=3.0, f16x3_scale_saturations=0)
    params = torch.randn(20_000_000, generator=torch.Generator().manual_seed(0))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), step, means, params)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(['step_loss.npy', 'step_idx_left.npy', 'step_accuracy.npy', 'epoch_loss.npy', 'epoch_accuracy.npy',
                            'epoch_num_codewords.npy', 'epoch_f16x3_scale_saturations.npy', 'params.npy'])
    total = 0
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, b), f                      # the sample is the same from run to run
        total += os.path.getsize(tmp_path / 'a' / f)
    assert total <= bench.DUMP_BUDGET_BYTES
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'step_idx_left.npy'), np.arange(12).reshape(6, 2))
    assert np.load(tmp_path / 'a' / 'step_idx_left.npy').dtype == np.float64
    p = np.load(tmp_path / 'a' / 'params.npy')
    assert 0 < p.size < params.numel() and p.dtype == np.float32
    assert np.isin(p[:1000], params.numpy()).all()         # a sample of the parameters themselves


def test_dump_outputs_keeps_small_sets_whole(tmp_path):
    bench = _bench()
    params = torch.randn(1000)
    bench.dump_outputs(str(tmp_path), torch.tensor(2.0), {'loss': 2.0}, params)
    assert sorted(os.listdir(tmp_path)) == ['epoch_loss.npy', 'params.npy', 'step.npy']
    np.testing.assert_array_equal(np.load(tmp_path / 'params.npy'), params.numpy())
