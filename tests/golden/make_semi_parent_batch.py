"""Generates tests/golden/semi_parent_batch.npz: what stage a (`train_semisup --device_data 40`) and stage c (`train_semisup_adv
--device_data 40`, ALTERNATE_BATCH) did BEFORE the device sampler t3d_semi_sample existed -- the name of every library call of a
two-step run and the first batch t3d_batch_assemble wrote -- on the NumPy specification library.  tests/test_semi_sampling_cpu.py holds
today's drivers to it: stage a with SEMI_SAMPLING_METHOD BATCH and SEMI_USE_LABELS2D_OF_CLASSES3D 0, or without
--SEMI_SAMPLING_METHOD, and stage c with ALTERNATE_BATCH and SEMI_USE_LABELS2D_OF_CLASSES3D 0, must emit exactly these launches.

Run on the commit whose behaviour is to be pinned: `python tests/golden/make_semi_parent_batch.py`.  The test module imports
`class_balanced_frustums`, `Recorder` and `STAGE_A_ARGV` from here, so the recording and the check see the same data set.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

from transferable3d_amd import dataset as _dataset      # noqa: E402
from transferable3d_amd.constants import MEAN_DIMS_ARR  # noqa: E402

_SYNTHETIC = _dataset.synthetic_frustums
OUT = os.path.join(HERE, 'semi_parent_batch.npz')
PER_CLASS = [3, 4, 5, 4, 3, 5, 4, 3, 5, 4]            # 40 frustums over the 10 classes, 3..5 of each
STAGE_A_ARGV = ['--SEMI_MODEL', 'A', '--WEAK_WEIGHT_REPROJECTION', '0', '--WEAK_WEIGHT_SURFACE', '0', '--num_point', '128',
                '--batch_size', '8', '--num_channels', '4', '--max_epoch', '1', '--steps_per_epoch', '2', '--device_data', '40']
STAGE_C_ARGV = ['--SEMI_MODEL', 'F', '--BOX_PC_MASK_REPRESENTATION', 'A', '--use_one_hot', '--SEMI_TRAIN_BOX_TRAIN_CLASS_AG_TNET', '1',
                '--SEMI_TRAIN_BOX_TRAIN_CLASS_AG_BOX', '1', '--SEMI_BOXPC_FIT_ONLY_ON_2D_CLS', '1', '--WEAK_WEIGHT_INTRACLASSVAR', '2',
                '--WEAK_WEIGHT_REPROJECTION', '0', '--SEMI_MULTIPLIER_FOR_WEAK_LOSS', '0.05', '--num_point', '128', '--batch_size', '8',
                '--num_channels', '4', '--max_epoch', '1', '--steps_per_epoch', '2', '--device_data', '40']
BATCH_KEYS = ('pc', 'y_seg', 'y_center', 'y_orient_cls', 'y_orient_reg', 'y_dims_cls', 'y_dims_reg', 'one_hot', 'is_data_2D')


def class_balanced_frustums(n_frustums=40, num_channel=6, seed=0, min_points=150, max_points=400):
    """dataset.synthetic_frustums with the classes dealt out as PER_CLASS says (in a fixed shuffled order) and fewer points."""
    assert n_frustums == sum(PER_CLASS)
    host = _SYNTHETIC(n_frustums, num_channel, seed, min_points, max_points)
    cls = np.repeat(np.arange(10), PER_CLASS).astype(np.int32)
    cls = cls[np.random.RandomState(1234).permutation(n_frustums)]
    host['size'] = host['size'] - MEAN_DIMS_ARR[host['cls']] + MEAN_DIMS_ARR[cls]
    host['cls'] = cls
    return host


def _synthetic_for_drivers(n_frustums, num_channel=6, seed=0, min_points=400, max_points=3000):
    return class_balanced_frustums(n_frustums, num_channel, seed)


def patch_driver_data(setattr_fn):
    """Makes `--device_data 40` of the drivers open the class-balanced data set.  setattr_fn: monkeypatch.setattr or setattr."""
    setattr_fn(_dataset, 'synthetic_frustums', _synthetic_for_drivers)


class Recorder:
    """Stands in front of a library object: the name of every t3d_* call in order, the batch behind every t3d_batch_assemble."""

    def __init__(self, lib):
        self._lib, self.names, self.batches = lib, [], []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('t3d_') or not callable(fn):
            return fn

        def call(*a):
            rc = fn(*a)
            self.names.append(name)
            if name == 't3d_batch_assemble' and rc == 0:
                self.batches.append(self.snapshot(a[0]))
            return rc
        return call

    @staticmethod
    def snapshot(a):
        from fake_t3d import arr
        p = a._obj if hasattr(a, '_obj') else a.contents
        B, N, ld = p.B, p.N, (p.ld_pc if p.ld_pc > 0 else p.C)
        flags = p.is_data_2D if p.is_data_2D else p.slot_is_2D
        return dict(pc=arr(p.pc, B, N, ld).copy(), y_seg=arr(p.y_seg, B, N).copy(), y_center=arr(p.y_center, B, 3).copy(),
                    y_orient_cls=arr(p.y_orient_cls, B).copy(), y_orient_reg=arr(p.y_orient_reg, B).copy(),
                    y_dims_cls=arr(p.y_dims_cls, B).copy(), y_dims_reg=arr(p.y_dims_reg, B, 3).copy(),
                    one_hot=arr(p.one_hot, B, 10).copy(), is_data_2D=arr(flags, B).copy(),
                    sample=arr(p.sample, B).copy() if p.sample_len == 0 else None)      # (the explicit-sample mode: a sampler ran before)


def run_stage_a(lib, extra_argv=(), logs=None):
    """Two steps of stage a on `lib` behind a Recorder; returns the recorder."""
    from transferable3d_amd.engine import Runtime
    from transferable3d_amd.train_semisup import build_flags, train
    rec = Recorder(lib)
    with tempfile.TemporaryDirectory() as tmp:
        flags = build_flags(STAGE_A_ARGV + ['--log_dir', tmp] + list(extra_argv))
        train(flags, rt=Runtime(device='cpu', lib=rec), log=(logs.append if logs is not None else (lambda *a: None)))
    return rec


def run_stage_c(lib, extra_argv=(), logs=None):
    """Two batch indices (four steps under ALTERNATE_BATCH) of stage c on `lib` behind a Recorder; returns (recorder, loss)."""
    from transferable3d_amd import train_semisup_adv as T
    from transferable3d_amd.engine import Runtime
    rec = Recorder(lib)
    with tempfile.TemporaryDirectory() as tmp:
        flags = T.build_flags(STAGE_C_ARGV + ['--log_dir', tmp] + list(extra_argv))
        _, loss = T.train(flags, rt=Runtime(device='cpu', lib=rec), log=(logs.append if logs is not None else (lambda *a: None)))
    return rec, loss


def main():
    from fake_t3d import FakeLib
    patch_driver_data(setattr)
    rec = run_stage_a(FakeLib())
    rec_c, _ = run_stage_c(FakeLib())
    first, first_c = rec.batches[0], rec_c.batches[0]
    np.savez_compressed(OUT, names=np.array(json.dumps(rec.names)), c_names=np.array(json.dumps(rec_c.names)),
                        **{k: first[k] for k in BATCH_KEYS}, **{'c_' + k: first_c[k] for k in BATCH_KEYS})
    for tag, r in (('stage a', rec), ('stage c', rec_c)):
        print('%s, %s: %d calls, %d batches, is_data_2D of the first batch %s' % (OUT, tag, len(r.names), len(r.batches),
                                                                                  r.batches[0]['is_data_2D']))


if __name__ == '__main__':
    main()
