"""CPU (NumPy specification library): what `bench.py --dump-outputs DIR` writes -- the end points and the updated variables of the
step it timed, as float32 .npy files within the 64 MB budget, identical for two runs on the same seeded inputs; the seeded sample
that keeps a larger output inside the budget."""
import os

import numpy as np
import pytest

from fake_t3d import FakeLib
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.setenv('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # (bench.py sets it when imported; restored after the test)
    monkeypatch.syspath_prepend(ROOT)
    import bench as b
    return b


def _two_steps(workload):
    from transferable3d_amd.step import build_training_step
    from transferable3d_amd.synthetic import make_batch
    B, N, C = 4, 128, 4
    g, model, step, loss = build_training_step(Runtime(device='cpu', lib=FakeLib()), workload, B, N, C, inline_dropout=True,
                                               dropout_seed=1234, seed=0)
    model.inputs.load(make_batch(B, N, C, seed=1234, boxpc=workload == 'boxpc'))
    for _ in range(2):
        step.run()
    return g, model, loss


@pytest.mark.parametrize('workload', ['A', 'boxpc'])
def test_dump_writes_the_step_outputs_and_repeats_them(bench, tmp_path, workload):
    g, model, loss = _two_steps(workload)
    bench.dump_outputs(str(tmp_path / 'a'), model, g.vars)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert {'loss.npy', 'weights.npy', 'grads.npy', 'moving_stats.npy'} <= set(files)
    got = {f[:-4]: np.load(tmp_path / 'a' / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    assert got['loss'].reshape(-1)[0] == np.float32(loss.reshape(-1)[0].item())
    assert np.array_equal(got['weights'], g.vars.params[:g.vars.used].numpy())
    assert np.array_equal(got['grads'], g.vars.grads[:g.vars.used].numpy())
    assert np.abs(got['grads']).max() > 0
    g2, model2, _ = _two_steps(workload)
    bench.dump_outputs(str(tmp_path / 'b'), model2, g2.vars)
    assert sorted(os.listdir(tmp_path / 'b')) == files
    for f in files:
        assert np.array_equal(np.load(tmp_path / 'b' / f), got[f[:-4]]), f


def test_fit_budget_keeps_a_fixed_sample_within_the_budget(bench):
    rs = np.random.RandomState(7)
    big, small = rs.standard_normal(100000).astype(np.float32), rs.standard_normal(1000).astype(np.float32)
    out = bench.fit_budget({'big': big.copy(), 'small': small.copy()}, budget=100000)
    assert sum(a.nbytes for a in out.values()) <= 100000
    assert np.array_equal(out['small'], small) and 0 < out['big'].size < big.size
    assert np.isin(out['big'], big).all()
    again = bench.fit_budget({'big': big.copy(), 'small': small.copy()}, budget=100000)
    assert np.array_equal(again['big'], out['big'])
    untouched = bench.fit_budget({'big': big.copy()}, budget=big.nbytes)
    assert np.array_equal(untouched['big'], big)
