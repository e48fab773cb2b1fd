"""GPU: t3d_semi_sample (csrc/data.hip) on the MI355X against its NumPy specification (tests/fake_semi_sample.py) -- bit-equal on
`sample` and `is_data_2D`, inside a captured graph whose step counter advances on the device -- and the sampler in front of
t3d_batch_assemble and of a training step."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import fake_semi_sample as S
import test_semi_sampling_cpu as T
from fake_semi_sample import FakeSemiLib
from transferable3d_amd import abi
from transferable3d_amd.dataset import DeviceFrustumSet
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu

STEPS = 64
F_BIG = 700


def big_host():
    """700 one-point frustums: 256 of them in the TRAIN_CLS classes (so that B = 256 under ALTERNATE_BATCH asks the 3-D list for every
    one of its members: len == count), one class ('bathtub') with a single member."""
    r = np.random.RandomState(3)
    train_no_tub = [c for c in T.TRAIN_IDS if c != 9]
    cls = np.concatenate([[9], r.choice(train_no_tub, 255), r.choice(T.TEST_IDS, F_BIG - 256)]).astype(np.int32)
    cls = cls[r.permutation(F_BIG)]
    z = np.zeros
    return dict(points=r.normal(size=(F_BIG, 6)).astype(np.float32), seg=z(F_BIG, np.int32), offsets=np.arange(F_BIG + 1),
                frustum_angle=z(F_BIG), box_center=z((F_BIG, 3)), heading=z(F_BIG), size=np.ones((F_BIG, 3)), cls=cls)


BIG = big_host()


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.fixture(scope='module')
def cpu():
    return Runtime(device='cpu', lib=FakeSemiLib())


def lists_of(rt_, classes3d, classes2d, shuffle_seed=9):
    ds = DeviceFrustumSet(rt_, **BIG).semi_lists(classes3d, classes2d)
    ds.shuffle(shuffle_seed)
    return ds


def replay_steps(rt, sampler, first_step, steps):
    """One eager launch, one captured graph, `steps` replays; the counter is advanced by a device-side add between them."""
    sampler.hyper[0] = float(first_step)
    assert rt.lib.t3d_semi_sample(C.byref(sampler.args), rt.stream()) == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        assert rt.lib.t3d_semi_sample(C.byref(sampler.args), rt.stream()) == 0
    out = torch.zeros(steps, 2, sampler.B, dtype=torch.int32, device=rt.device)
    sampler.hyper[0] = float(first_step)
    for k in range(steps):
        g.replay()
        out[k, 0].copy_(sampler.sample)
        out[k, 1].copy_(sampler.flag)
        sampler.hyper[0:1].add_(1.0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


CASES = [('BATCH', 0.0, b) for b in (2, 8, 32, 256)] + \
        [(m, p, b) for m in ('ALTERNATE_BATCH', 'MIXED_BATCH') for p in (0.0, 1.0, 0.5) for b in (2, 8, 32, 256)]


@pytest.mark.parametrize('method,prob,batch', CASES, ids=lambda v: str(v))
def test_sampler_is_bit_equal_to_the_specification_over_64_captured_steps(method, prob, batch, rt, cpu):
    """Dual membership (the 2-D list holds every class), 256 frustums in the 3-D list, one class with a single member."""
    classes2d = T.TRAIN_IDS + T.TEST_IDS
    got = replay_steps(rt, T.Sampler(rt, lists_of(rt, T.TRAIN_IDS, classes2d), method, batch=batch, prob=prob, seed=21), 3, STEPS)
    ref = T.Sampler(cpu, lists_of(cpu, T.TRAIN_IDS, classes2d), method, batch=batch, prob=prob, seed=21)
    for k in range(STEPS):
        ids, flags = ref(3 + k)
        assert np.array_equal(got[k, 0], ids) and np.array_equal(got[k, 1], flags), (method, prob, batch, 'step', 3 + k)
    if method == 'ALTERNATE_BATCH' and batch == 256 and prob == 0.0:      # len == count: every odd step is a permutation of the list
        members = np.sort(np.nonzero(np.isin(BIG['cls'], T.TRAIN_IDS))[0])
        assert all(np.array_equal(np.sort(got[k, 0]), members) for k in range(0, STEPS, 2))          # (first step 3: odd)


def test_batch_with_an_empty_3d_list(rt, cpu):
    got = replay_steps(rt, T.Sampler(rt, lists_of(rt, [], T.TEST_IDS), 'BATCH', batch=32), 0, STEPS)
    ref = T.Sampler(cpu, lists_of(cpu, [], T.TEST_IDS), 'BATCH', batch=32)
    for k in range(STEPS):
        ids, flags = ref(k)
        assert np.array_equal(got[k, 0], ids) and np.array_equal(got[k, 1], flags) and flags.all()


def test_replaying_from_the_same_counter_gives_the_same_batch(rt):
    s = T.Sampler(rt, lists_of(rt, T.TRAIN_IDS, T.TEST_IDS), 'MIXED_BATCH', batch=32, prob=0.5, seed=2)
    a, b = replay_steps(rt, s, 10, 8), replay_steps(rt, s, 10, 8)
    assert np.array_equal(a, b) and not np.array_equal(a[0], a[1])


def test_the_launcher_refuses_what_the_specification_refuses(rt):
    ds = T.make_ds(rt, labels2d_of_classes3d=False)
    assert T.Sampler(rt, ds, 'MIXED_BATCH', batch=7).launch(0) == -2
    assert T.Sampler(rt, ds, 'ALTERNATE_BATCH', batch=20, prob=0.5).launch(0) == -2
    assert T.Sampler(rt, ds, 'BATCH', batch=257).launch(0) == -2
    a = T.Sampler(rt, ds, 'BATCH').args
    a.struct_size -= 8
    assert rt.lib.t3d_semi_sample(C.byref(a), rt.stream()) == abi.ERR_ABI
    torch.cuda.synchronize()


def _assembled(rt_):
    """One MIXED batch of the 40-frustum data set: t3d_semi_sample, then t3d_batch_assemble reading its two outputs."""
    B, N, Cc = T.B, T.N, 4
    ds = T.make_ds(rt_)
    s = T.Sampler(rt_, ds, 'MIXED_BATCH', prob=0.5, seed=8)
    z = lambda *shape, dt=torch.float32: rt_.zeros(*shape, dtype=dt)
    x = types.SimpleNamespace(pc=z(B * N, Cc), y_seg=z(B * N, dt=torch.int32), y_center=z(B, 3), y_orient_cls=z(B, dt=torch.int32),
                              y_orient_reg=z(B), y_dims_cls=z(B, dt=torch.int32), y_dims_reg=z(B, 3), one_hot_vec=z(B, 10),
                              is_data_2D=s.flag)
    a = ds.assemble_args(x, s.hyper, B, N, Cc, seed=8, sample=s.sample)
    a.is_data_2D, a.frustum_is_2D, a.slot_is_2D = abi.iptr(None), abi.iptr(None), abi.iptr(s.flag)
    assert s.launch(6) == 0
    assert rt_.lib.t3d_batch_assemble(C.byref(a), rt_.stream()) == 0
    if rt_.device.type == 'cuda':
        torch.cuda.synchronize()
    return {k: getattr(x, k).cpu().numpy() for k in vars(x)}, s.sample.cpu().numpy()


def test_a_mixed_batch_is_assembled_as_the_specification_assembles_it(rt, cpu):
    got, ids = _assembled(rt)
    ref, ids_ref = _assembled(cpu)
    assert np.array_equal(ids, ids_ref) and got['is_data_2D'].tolist() == [1] * 4 + [0] * 4
    for k in ('is_data_2D', 'one_hot_vec', 'y_seg', 'y_dims_cls', 'y_orient_cls'):
        assert np.array_equal(got[k], ref[k]), k
    for k in ('pc', 'y_center', 'y_orient_reg', 'y_dims_reg'):
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=2e-5, err_msg=k)
    assert not got['y_center'][:4].any() and got['y_center'][4:].any()


def test_a_mixed_batch_follows_the_oracle_on_the_device(hip_lib, monkeypatch):
    monkeypatch.setattr(T, '_runtime', lambda: Runtime(lib=hip_lib))
    monkeypatch.setattr(T, 'SHAPE', (8, 256))
    T.test_a_mixed_batch_follows_the_oracle('A', monkeypatch)
