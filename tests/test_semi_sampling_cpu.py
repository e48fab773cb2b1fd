"""CPU (NumPy specification library, tests/fake_semi_sample.py): SEMI_SAMPLING_METHOD and SEMI_USE_LABELS2D_OF_CLASSES3D -- the sampler
t3d_semi_sample, DeviceFrustumSet.semi_lists / partition / shuffle, and the two drivers through it.  The data set is 40 synthetic
frustums over the 10 classes, 3..5 of each (tests/golden/make_semi_parent_batch.py); TRAIN_CLS / TEST_CLS are the defaults (19 / 21
frustums); B = 8, N = 128."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import fake_semi_sample as S
from fake_semi_sample import FakeSemiLib
from transferable3d_amd import abi
from transferable3d_amd.config import make_parser
from transferable3d_amd.constants import type2class
from transferable3d_amd.dataset import DeviceFrustumSet, synthetic_cameras
from transferable3d_amd.engine import Runtime

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_semi_parent_batch', os.path.join(GOLDEN, 'make_semi_parent_batch.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

B, N = 8, 128
_F = make_parser().parse_special_args([])
TRAIN_IDS = [type2class[t] for t in _F.SUNRGBD_SEMI_TRAIN_CLS]
TEST_IDS = [type2class[t] for t in _F.SUNRGBD_SEMI_TEST_CLS]
HOST = G.class_balanced_frustums()
CLS = HOST['cls']
METHODS = ('BATCH', 'ALTERNATE_BATCH', 'MIXED_BATCH')


def _runtime():
    """tests/test_semi_sampling_gpu.py replaces this factory with the HIP library."""
    return Runtime(device='cpu', lib=FakeSemiLib())


def make_ds(rt, labels2d_of_classes3d=True, host=HOST):
    ds = DeviceFrustumSet(rt, **host).set_camera(**synthetic_cameras(len(host['cls'])))
    return ds.semi_lists(TRAIN_IDS, TRAIN_IDS + TEST_IDS if labels2d_of_classes3d else TEST_IDS)


class Sampler:
    """One argument struct of t3d_semi_sample on `rt` and its buffers."""

    def __init__(self, rt, ds, method, batch=B, prob=0.0, seed=5):
        self.rt, self.B = rt, batch
        self.hyper = rt.zeros(4)
        self.sample, self.flag = rt.zeros(batch, dtype=torch.int32), rt.zeros(batch, dtype=torch.int32)
        self.args = ds.semi_sample_args(self.hyper, batch, self.sample, self.flag, method=method, seed=seed, equal_prob=prob)

    def launch(self, step):
        self.hyper[0] = float(step)
        return self.rt.lib.t3d_semi_sample(C.byref(self.args), self.rt.stream())

    def __call__(self, step):
        assert self.launch(step) == 0
        return self.sample.cpu().numpy().copy(), self.flag.cpu().numpy().copy()


def _walk(ds, rt, steps):
    s = Sampler(rt, ds, 'BATCH')
    out = [s(k) for k in range(steps)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def test_batch_walks_both_lists_every_3d_class_frustum_twice():
    """BATCH with SEMI_USE_LABELS2D_OF_CLASSES3D: an epoch is len3D + len2D entries long; every TRAIN_CLS frustum appears once per flag
    value, every TEST_CLS frustum once with flag 1; a new shuffle changes the order, not the multiset."""
    rt = _runtime()
    ds = make_ds(rt)
    len3d, len2d = int(np.isin(CLS, TRAIN_IDS).sum()), len(CLS)
    assert (len(ds.semi[0]['host']), len(ds.semi[1]['host']), ds.semi_len) == (len3d, len2d, len3d + len2d) == (19, 40, 59)
    # the whole permutation: ceil((len3D + len2D) / B) steps, the positions behind the end wrap around
    ds.shuffle(1)
    ids, flags = _walk(ds, rt, -(-ds.semi_len // B))
    pairs = sorted(zip(ids[:ds.semi_len].tolist(), flags[:ds.semi_len].tolist()))
    expect = sorted([(f, 0) for f in range(len(CLS)) if CLS[f] in TRAIN_IDS] + [(f, 1) for f in range(len(CLS))])
    assert pairs == expect
    assert np.array_equal(ids[ds.semi_len:], ids[:len(ids) - ds.semi_len])
    ds.shuffle(2)
    ids2, flags2 = _walk(ds, rt, -(-ds.semi_len // B))
    assert sorted(zip(ids2[:ds.semi_len].tolist(), flags2[:ds.semi_len].tolist())) == expect
    assert not np.array_equal(ids2[:ds.semi_len], ids[:ds.semi_len])
    # partition: whole batches only, floor((len3D + len2D) / B) steps; no entry twice inside the pass, the walk wraps at its end
    ds = make_ds(rt)
    n = ds.partition(0, 1, B)
    assert n == (len3d + len2d) // B == 7 and ds.walk_len == n * B
    ds.shuffle(1)
    ids, flags = _walk(ds, rt, n + 1)
    pass_pairs = list(zip(ids[:n * B].tolist(), flags[:n * B].tolist()))
    assert len(set(pass_pairs)) == n * B and set(pass_pairs) <= set(expect)
    assert np.array_equal(ids[n * B:], ids[:B]) and np.array_equal(flags[n * B:], flags[:B])
    # two replicas: disjoint slices of the common permutation
    a, b = make_ds(rt), make_ds(rt)
    assert a.partition(0, 2, B) == b.partition(1, 2, B) == (len3d + len2d) // 2 // B
    a.shuffle(3), b.shuffle(3)
    pa, pb = a.semi_perm[:a.walk_len].cpu().numpy(), b.semi_perm[:b.walk_len].cpu().numpy()
    assert not set(pa.tolist()) & set(pb.tolist())
    # without semi lists partition counts frustums, as before
    assert DeviceFrustumSet(rt, **HOST).partition(0, 1, B) == len(CLS) // B


def test_batch_with_an_empty_3d_list_flags_everything_2d():
    rt = _runtime()
    ds = DeviceFrustumSet(rt, **HOST).semi_lists([], TEST_IDS)
    ds.shuffle(4)
    ids, flags = _walk(ds, rt, 2)
    assert flags.all() and np.isin(CLS[ids], TEST_IDS).all()


@pytest.mark.parametrize('prob', [0.0, 1.0])
def test_alternate_batch_draws_the_2d_list_on_even_and_the_3d_list_on_odd_steps(prob):
    rt = _runtime()
    ds = make_ds(rt, labels2d_of_classes3d=False)
    s = Sampler(rt, ds, 'ALTERNATE_BATCH', prob=prob)
    for step in range(6):
        ids, flags = s(step)
        assert (flags == (1 if step % 2 == 0 else 0)).all()
        assert np.isin(CLS[ids], TEST_IDS if step % 2 == 0 else TRAIN_IDS).all()
        if prob == 0.0:
            assert len(set(ids.tolist())) == B                          # np.random.choice(len, B, replace=False)
        else:
            # np.array_split([1] * 8, 5): {2, 2, 2, 1, 1}, laid out class after class
            counts = np.bincount(CLS[ids], minlength=10)
            assert sorted(counts[counts > 0].tolist()) == [1, 1, 2, 2, 2]
            assert (np.diff(CLS[ids]) >= 0).all()


@pytest.mark.parametrize('prob', [0.0, 1.0])
def test_mixed_batch_is_half_2d_half_3d(prob):
    rt = _runtime()
    ds = make_ds(rt)
    s = Sampler(rt, ds, 'MIXED_BATCH', prob=prob)
    for step in range(4):
        ids, flags = s(step)
        assert flags.tolist() == [1] * 4 + [0] * 4
        assert np.isin(CLS[ids[4:]], TRAIN_IDS).all()                      # (the 2-D list holds every class here)
        if prob == 0.0:
            assert len(set(ids[:4].tolist())) == 4 and len(set(ids[4:].tolist())) == 4
        else:
            assert sorted(np.bincount(CLS[ids[4:]], minlength=10)[TRAIN_IDS].tolist()) == [0, 1, 1, 1, 1]      # 4 slots over 5 classes
    ds2 = make_ds(rt, labels2d_of_classes3d=False)
    ids, _ = Sampler(rt, ds2, 'MIXED_BATCH')(0)
    assert np.isin(CLS[ids[:4]], TEST_IDS).all() and np.isin(CLS[ids[4:]], TRAIN_IDS).all()


def test_shapes_the_sampler_refuses():
    rt = _runtime()
    ds = make_ds(rt, labels2d_of_classes3d=False)
    assert Sampler(rt, ds, 'MIXED_BATCH', batch=7).launch(0) == -2                 # sample_mixed asserts bsize % 2 == 0
    assert Sampler(rt, ds, 'ALTERNATE_BATCH', batch=20, prob=0.0).launch(0) == -2  # 19 frustums with 3-D labels: numpy raises too
    assert Sampler(rt, ds, 'ALTERNATE_BATCH', batch=20, prob=0.5).launch(0) == -2  # the coin can come up false
    assert Sampler(rt, ds, 'ALTERNATE_BATCH', batch=20, prob=1.0).launch(0) == 0   # with replacement inside the classes
    assert Sampler(rt, ds, 'ALTERNATE_BATCH', batch=19, prob=0.0).launch(1) == 0
    assert Sampler(rt, ds, 'MIXED_BATCH', batch=40, prob=0.0).launch(0) == -2
    assert Sampler(rt, ds, 'BATCH', batch=257).launch(0) == -2
    with pytest.raises(ValueError, match='unknown SEMI_SAMPLING_METHOD'):
        Sampler(rt, ds, 'ALTERNATING')
    a = Sampler(rt, ds, 'BATCH').args
    a.struct_size -= 8
    assert rt.lib.t3d_semi_sample(C.byref(a), rt.stream()) == abi.ERR_ABI


def test_whole_list_without_replacement_is_a_permutation():
    """len == count: the edge of the draw without replacement."""
    rt = _runtime()
    ds = make_ds(rt, labels2d_of_classes3d=False)
    s = Sampler(rt, ds, 'ALTERNATE_BATCH', batch=19)
    seen = set()
    for step in (1, 3, 5):
        ids, _ = s(step)
        assert sorted(ids.tolist()) == sorted(np.nonzero(np.isin(CLS, TRAIN_IDS))[0].tolist())
        seen.add(tuple(ids.tolist()))
    assert len(seen) == 3


def test_sampler_size_follows_the_header(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / 's.c'
    src.write_text('#include <stdio.h>\n#include "t3d.h"\nint main(void) { printf("%zu %d\\n", sizeof(t3d_semi_sample_args), '
                   'T3D_V2_SIZE_semi_sample_args); return 0; }\n')
    subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), str(src), '-o', str(tmp_path / 's')])
    size, v2 = (int(v) for v in subprocess.check_output([str(tmp_path / 's')], text=True).split())
    assert size == v2 == C.sizeof(abi.SemiSampleArgs) and abi.SemiSampleArgs().struct_size == size


def test_coin_and_class_assignment_frequencies():
    """2 000 steps of the specification at prob = 0.5: the coin within 4 sigma of a binomial; every class takes the larger group with
    frequency (n % k) / k within 4 sigma."""
    steps, seed = 2000, 11
    heads = sum(S.coin(seed, k, 0.5) for k in range(steps))
    assert abs(heads - 0.5 * steps) < 4 * np.sqrt(steps * 0.25)
    n, k = 8, 5
    larger = np.zeros(k)
    for step in range(steps):
        sizes = S.group_sizes(S.half_key(seed, step, True), n, k)
        assert sorted(sizes) == [1, 1, 2, 2, 2]
        larger += np.array(sizes) == 2
    p = (n % k) / k
    assert (np.abs(larger - p * steps) < 4 * np.sqrt(steps * p * (1 - p))).all()
    # and the sampler takes the coin it is specified to take
    rt = Runtime(device='cpu', lib=FakeSemiLib())
    s = Sampler(rt, make_ds(rt, labels2d_of_classes3d=False), 'ALTERNATE_BATCH', prob=0.5, seed=seed)
    for step in range(0, 40, 2):
        ids, _ = s(step)
        if S.coin(seed, step, 0.5):
            assert sorted(np.bincount(CLS[ids], minlength=10)[TEST_IDS].tolist()) == [1, 1, 2, 2, 2] and (np.diff(CLS[ids]) >= 0).all()
        else:
            assert len(set(ids.tolist())) == B


# ---- drivers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('argv', [['--SEMI_SAMPLING_METHOD', 'BATCH', '--SEMI_USE_LABELS2D_OF_CLASSES3D', '0'], []],
                         ids=['BATCH+labels2d=0', 'no-flag'])
def test_stage_a_emits_the_parent_commits_launches(argv, monkeypatch):
    """SEMI_SAMPLING_METHOD BATCH with SEMI_USE_LABELS2D_OF_CLASSES3D 0, and a command line without the flag (the parsed default is
    ALTERNATE_BATCH; stage a has always run BATCH): every library call and the first batch are the parent commit's."""
    G.patch_driver_data(monkeypatch.setattr)
    logs = []
    rec = G.run_stage_a(FakeSemiLib(), argv, logs)
    _against_golden(rec, '')
    said = [l for l in logs if 'stage a runs BATCH' in l]
    assert len(said) == (0 if argv else 1)


def _flags_of(rec):
    return [b['is_data_2D'].tolist() for b in rec.batches]


def _against_golden(rec, prefix):
    z = np.load(os.path.join(GOLDEN, 'semi_parent_batch.npz'))
    names = json.loads(str(z[prefix + 'names']))
    assert rec.names == names and 't3d_semi_sample' not in names
    for k in G.BATCH_KEYS:
        want = z[prefix + k]
        if want.dtype.kind == 'i':
            assert np.array_equal(rec.batches[0][k], want), k
        else:
            np.testing.assert_allclose(rec.batches[0][k], want, rtol=0, atol=1e-6, err_msg=k)


def _expected_batches(method, labels2d, steps, driver_seed=0):
    """What the specification draws for the drivers' first `steps` steps (FLAGS.seed = 0, one replica, --steps_per_epoch 2,
    SEMI_SAMPLE_EQUAL_CLASS_WITH_PROB 0): [(sample, is_data_2D)]."""
    lists = [dict(ids=np.nonzero(np.isin(CLS, ids))[0].astype(np.int32), n_groups=0, members=None, offsets=None)
             for ids in (TRAIN_IDS, TRAIN_IDS + TEST_IDS if labels2d else TEST_IDS)]
    total = sum(len(l['ids']) for l in lists)
    walk = min(total // B, 2) * B                                            # partition(0, 1, B, steps_per_epoch=2)
    perm = np.random.RandomState(driver_seed * 1000003 + 0).permutation(total)[:walk]      # shuffle of epoch 0
    seed = (driver_seed * 7919 + 0) ^ 0x2545F491                             # use_device_dataset(seed=...), nets.emit_batch_assemble
    return [S.semi_sample_spec(abi.SEMI_METHODS[method], lists[0], lists[1], B, seed, k, 0.0, perm, walk) for k in range(steps)]


def _check_method(method, rec, labels2d):
    """The frustums and the is_data_2D flags every step consumed are the ones the method draws."""
    steps = 4 if method == 'ALTERNATE_BATCH' else 2
    assert len(rec.batches) == steps
    for k, (ids, flags) in enumerate(_expected_batches(method, labels2d, steps)):
        got = rec.batches[k]
        assert np.array_equal(got['sample'], ids) and np.array_equal(got['is_data_2D'], flags), (method, labels2d, k)
        assert np.array_equal(np.argmax(got['one_hot'], 1), CLS[ids])
        assert np.isin(CLS[ids[flags == 0]], TRAIN_IDS).all() and (labels2d or np.isin(CLS[ids[flags == 1]], TEST_IDS).all())
    flags = _flags_of(rec)
    if method == 'ALTERNATE_BATCH':
        assert flags == [[1] * B, [0] * B] * 2
    elif method == 'MIXED_BATCH':
        assert flags == [[1] * 4 + [0] * 4] * 2
    else:
        assert {f for fl in flags for f in fl} == {0, 1}


# (BATCH without the labels-2D flag is the parent commit's path: test_stage_a_emits_the_parent_commits_launches)
@pytest.mark.parametrize('method,labels2d', [(m, l) for m in METHODS for l in (1, 0) if (m, l) != ('BATCH', 0)])
def test_stage_a_honours_the_method_and_the_recipe_flags(method, labels2d, monkeypatch):
    """README recipe a: --SEMI_SAMPLING_METHOD ... --SEMI_USE_LABELS2D_OF_CLASSES3D 1 (and the methods without it)."""
    G.patch_driver_data(monkeypatch.setattr)
    logs = []
    rec = G.run_stage_a(FakeSemiLib(), ['--SEMI_SAMPLING_METHOD', method, '--SEMI_USE_LABELS2D_OF_CLASSES3D', str(labels2d)], logs)
    assert rec.names.count('t3d_semi_sample') == rec.names.count('t3d_batch_assemble') == (4 if method == 'ALTERNATE_BATCH' else 2)
    assert rec.names.index('t3d_semi_sample') + 1 == rec.names.index('t3d_batch_assemble')
    _check_method(method, rec, labels2d)
    assert any('SEMI_SAMPLING_METHOD %s on the device: 19 frustums with 3-D labels, %d with 2-D labels' % (method, 40 if labels2d else 21)
               in l for l in logs)
    for b in rec.batches:       # a 2-D slot carries no 3-D label
        two = b['is_data_2D'] == 1
        assert not b['y_seg'][two].any() and not b['y_center'][two].any() and b['one_hot'].sum(1).tolist() == [1.0] * B


def test_stage_a_takes_a_method_however_it_is_asked_for_and_refuses_an_unknown_one(monkeypatch, tmp_path):
    from transferable3d_amd.train_semisup import build_flags, requested_sampling_method, train
    G.patch_driver_data(monkeypatch.setattr)
    base = G.STAGE_A_ARGV + ['--log_dir', str(tmp_path)]
    assert requested_sampling_method(build_flags(base)) == (None, False)
    # every spelling argparse takes: the whole flag, `=`, an unambiguous abbreviation; the parser's own default value included
    for argv in (['--SEMI_SAMPLING_METHOD', 'ALTERNATE_BATCH'], ['--SEMI_SAMPLING_METHOD=ALTERNATE_BATCH'],
                 ['--SEMI_SAMPLING_M', 'ALTERNATE_BATCH']):
        assert requested_sampling_method(build_flags(base + argv)) == ('ALTERNATE_BATCH', True), argv
    # a caller that passes FLAGS: assigning the method asks for it, the parser's default value included
    flags = build_flags(base)
    flags.SEMI_SAMPLING_METHOD = 'ALTERNATE_BATCH'
    assert requested_sampling_method(flags) == ('ALTERNATE_BATCH', True)
    rec = G.Recorder(FakeSemiLib())
    train(flags, rt=Runtime(device='cpu', lib=rec), log=lambda *a: None)
    _check_method('ALTERNATE_BATCH', rec, 0)
    flags = build_flags(base)
    flags.SEMI_SAMPLING_METHOD = 'MIXED_BATCH'
    rec = G.Recorder(FakeSemiLib())
    train(flags, rt=Runtime(device='cpu', lib=rec), log=lambda *a: None)
    _check_method('MIXED_BATCH', rec, 0)
    for bad in (base + ['--SEMI_SAMPLING_METHOD', 'MIXED'], base + ['--SEMI_SAMPLING_M=BATCHES']):
        with pytest.raises(ValueError, match='unknown SEMI_SAMPLING_METHOD'):
            train(build_flags(bad), rt=Runtime(device='cpu', lib=FakeSemiLib()), log=lambda *a: None)


def test_contradictory_sampling_options_are_refused():
    from transferable3d_amd import api, semisup_v1_sunrgbd as MODEL
    rt = _runtime()
    with api.Graph(rt=rt).as_default() as g:
        MODEL.placeholder_inputs(B, N, 4)
        with pytest.raises(ValueError, match='semi_lists'):
            g.use_device_dataset(DeviceFrustumSet(rt, **HOST), semi_sampling='BATCH')
        with pytest.raises(ValueError, match='unknown SEMI_SAMPLING_METHOD'):
            g.use_device_dataset(make_ds(rt), semi_sampling='BATCHES')
        from transferable3d_amd.engine import Plan
        with pytest.raises(ValueError, match='exclude each other'):
            g.engine.emit_batch_assemble(Plan(rt), make_ds(rt), g.inputs, semi_sampling='MIXED_BATCH', alternate=True)


def test_stage_c_alternate_batch_emits_the_parent_commits_launches(monkeypatch):
    """ALTERNATE_BATCH with SEMI_USE_LABELS2D_OF_CLASSES3D 0 (the parser's defaults): every library call and the first batch of stage c
    are the parent commit's."""
    G.patch_driver_data(monkeypatch.setattr)
    for argv in ([], ['--SEMI_SAMPLING_METHOD', 'ALTERNATE_BATCH', '--SEMI_USE_LABELS2D_OF_CLASSES3D', '0']):
        rec, loss = G.run_stage_c(FakeSemiLib(), argv)
        assert np.isfinite(loss)
        _against_golden(rec, 'c_')
        assert _flags_of(rec) == [[1] * B, [0] * B] * 2


@pytest.mark.parametrize('method,labels2d', [('BATCH', 1), ('BATCH', 0), ('ALTERNATE_BATCH', 1), ('MIXED_BATCH', 0), ('MIXED_BATCH', 1)])
def test_stage_c_honours_the_method(method, labels2d, monkeypatch):
    """BATCH without SEMI_USE_LABELS2D_OF_CLASSES3D too: the TEST_CLS frustums are 2-D data (before t3d_semi_sample stage c ran them
    with their 3-D labels)."""
    G.patch_driver_data(monkeypatch.setattr)
    rec, loss = G.run_stage_c(FakeSemiLib(), ['--SEMI_SAMPLING_METHOD', method, '--SEMI_USE_LABELS2D_OF_CLASSES3D', str(labels2d)])
    assert np.isfinite(loss)
    assert rec.names.count('t3d_semi_sample') == rec.names.count('t3d_batch_assemble')
    _check_method(method, rec, labels2d)


def test_stage_c_refuses_an_unknown_method(monkeypatch):
    G.patch_driver_data(monkeypatch.setattr)
    with pytest.raises(ValueError, match='unknown SEMI_SAMPLING_METHOD'):
        G.run_stage_c(FakeSemiLib(), ['--SEMI_SAMPLING_METHOD', 'EVERY_OTHER'])


# ---- a batch with both flag values through the strong / weak masks ------------------------------------------------------------------
SHAPE = (B, N)


def mixed_trajectory_batch(workload, batch, n_points, channels, seed):
    """model_check.trajectory_batch with the classes and the flags of a MIXED batch the specification draws from the data set."""
    from transferable3d_amd.synthetic import make_batch
    b = make_batch(batch, n_points, channels, seed=seed, boxpc=False)
    lists = [dict(ids=np.nonzero(np.isin(CLS, ids))[0].astype(np.int32), n_groups=0, members=None, offsets=None)
             for ids in (TRAIN_IDS, TRAIN_IDS + TEST_IDS)]
    sample, flag = S.semi_sample_spec(abi.SEMI_MIXED_BATCH, lists[0], lists[1], batch, seed=7, step=seed, equal_prob=0.0)
    cls = CLS[sample]
    b['one_hot_vec'] = np.eye(10, dtype=np.float32)[cls]
    b['y_dims_cls'] = cls.astype(np.int32)
    b['is_data_2D'] = flag.astype(np.int32)
    assert flag.tolist() == [1] * (batch // 2) + [0] * (batch // 2)
    return b


@pytest.mark.parametrize('workload', ['A', 'F'])
def test_a_mixed_batch_follows_the_oracle(workload, monkeypatch):
    """Two training steps on a batch whose first half is 2-D data and second half 3-D data: heads, loss and updated weights against
    oracle/ref_torch.py within trajectory_check's own bounds."""
    import model_check
    monkeypatch.setattr(model_check, 'trajectory_batch', mixed_trajectory_batch)
    rep = model_check.trajectory_check(_runtime(), workload, steps=2, B=SHAPE[0], N=SHAPE[1])
    assert all(r['weight_entries_checked'] > 1000 for r in rep[:-1])
