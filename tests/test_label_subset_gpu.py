"""GPU: t3d_label_subset (csrc/data.hip k_label_subset) on the MI355X against its NumPy specification (tests/fake_label_subset.py) --
every output exact --, the lists it builds in front of t3d_semi_sample on the recorded frustum file held in HBM, and the drivers'
--train_data3D_keep_prob / --classes_to_drop_prob on the device.  The scan walks chunks of 1024 frustums."""
import ctypes as C

import numpy as np
import pytest
import torch

import fake_label_subset as L
import test_label_subset_cpu as P
import test_semi_sampling_cpu as T
from transferable3d_amd import abi, train_boxpc, train_semisup
from transferable3d_amd.dataset import DeviceFrustumSet, reference_label_subset
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu
CHUNK = 1024
Z = P.Z
TRAIN_IDS, TEST_IDS = [P.NAMES.index(t) for t in P.CLASSES3D], [P.NAMES.index(t) for t in P.CLASSES2D]


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


def launch(rt, cls, member=None, mask=None, keep=1.0, add=-1.0, seed=20, F=None):
    """One launch on fresh buffers (pre-filled with a pattern, so that every element the kernel owes is seen to be written)."""
    dev = rt.device
    F = len(cls) if F is None else F
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    t = dict(cls=up(cls, np.int32), member=up(member, np.uint8), mask=up(mask, np.int32))
    out = {k: torch.full((n,), 0x7f7f7f7f, dtype=torch.int32, device=dev)
           for k, n in (('ids', max(F, 1)), ('members', max(F, 1)), ('offsets', 11), ('present', 10), ('summary', 4))}
    a = abi.LabelSubsetArgs()
    a.F, a.cls, a.member, a.class_mask = F, abi.iptr(t['cls']), abi.u8ptr(t['member']), abi.iptr(t['mask'])
    a.keep_prob, a.add_prob, a.seed = keep, add, seed
    a.ids, a.members, a.offsets, a.present, a.summary = (abi.iptr(out[k]) for k in ('ids', 'members', 'offsets', 'present', 'summary'))
    rc = rt.lib.t3d_label_subset(C.byref(a), rt.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def check(rt, cls, member=None, mask=None, keep=1.0, add=-1.0, seed=20):
    rc, got = launch(rt, cls, member, mask, keep, add, seed)
    assert rc == 0
    spec = L.label_subset_spec(cls, member, mask, keep, add, seed)
    for k in ('ids', 'members', 'offsets', 'present'):
        assert np.array_equal(got[k], spec[k]), (k, len(cls))
    assert got['summary'].tolist() == [spec['len'], spec['n_groups'], 0, 0]
    return got, spec


def classes_one_empty(F, seed):
    return np.random.RandomState(seed).choice([c for c in range(10) if c != 4], size=F).astype(np.int32)


@pytest.mark.parametrize('F', [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 37])
def test_flags_against_the_specification(F, rt):
    """10 classes with one empty, random flags; flags all 0 and all 1; the same input twice gives the same bytes."""
    cls = classes_one_empty(F, F)
    member = (np.random.RandomState(F + 1).uniform(size=F) < 0.5).astype(np.uint8)
    got, spec = check(rt, cls, member)
    assert spec['present'][4] == 0
    again = launch(rt, cls, member)[1]
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    _, zero = check(rt, cls, np.zeros(F, np.uint8))
    assert zero['len'] == 0 and zero['n_groups'] == 0 and not zero['offsets'].any()
    _, ones = check(rt, cls, np.ones(F, np.uint8))
    assert ones['len'] == F and np.array_equal(ones['ids'], np.arange(F))


@pytest.mark.parametrize('F', [65, CHUNK + 1, 3 * CHUNK + 37])
def test_hash_draws_against_the_specification(F, rt):
    cls = classes_one_empty(F, 7 * F)
    mask = np.isin(np.arange(10), TRAIN_IDS).astype(np.int32)
    _, none = check(rt, cls, mask=mask, keep=0.0, add=-1.0)                      # keep = 0: nothing of the masked classes
    assert none['len'] == 0
    _, every = check(rt, cls, mask=mask, keep=1.0, add=-1.0)                     # keep = 1: everything of the masked classes
    assert np.array_equal(every['ids'][:every['len']], np.nonzero(mask[cls])[0])
    _, some = check(rt, cls, mask=mask, keep=0.5, add=0.25, seed=3)
    assert 0 < some['len'] < F


def test_hash_draws_keep_half_and_follow_the_seed(rt):
    """F = 4096 frustums of one class, keep = 0.5: the kept share is binomial, sigma = sqrt(0.25 / 4096); 5 sigma = 0.039."""
    F = 4096
    cls, mask = np.full(F, 2, np.int32), np.ones(10, np.int32)
    a = check(rt, cls, mask=mask, keep=0.5, seed=20)[1]
    b = check(rt, cls, mask=mask, keep=0.5, seed=21)[1]
    share = a['len'] / F
    print('kept share at keep = 0.5: %.4f (seed 21: %.4f)' % (share, b['len'] / F))
    assert abs(share - 0.5) <= 5 * np.sqrt(0.25 / F)
    assert not np.array_equal(a['ids'], b['ids'])


def test_what_the_launcher_refuses(rt):
    cls = classes_one_empty(70, 1)
    assert launch(rt, cls, np.ones(70, np.uint8), F=0)[0] == -2
    assert launch(rt, cls, np.ones(70, np.uint8), F=-5)[0] == -2
    assert launch(rt, cls)[0] == -1                                               # neither flags nor a class mask
    bad = cls.copy()
    bad[69] = 10
    rc, got = launch(rt, bad, np.ones(70, np.uint8))
    assert rc == -1 and got['summary'].tolist() == [0, 0, 1, 0]
    bad[69] = -1
    assert launch(rt, bad, mask=np.ones(10, np.int32))[0] == -1


# ---- the recorded frustum file held in HBM --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixture_lists(rt):
    ds = DeviceFrustumSet.from_pickle(rt, P.FIXTURE)
    member = reference_label_subset(ds.class_names, P.CLASSES3D, 0.5, 0.25)
    return ds.semi_lists(TRAIN_IDS, TEST_IDS, member3d=member)


def test_lists_and_groups_of_the_fixture_are_the_recorded_ones(fixture_lists):
    ds, k = fixture_lists, P.semi_key(0.5, 0.25)
    for l, idx, m in zip(ds.semi, ('idx_3Dl', 'idx_2Dl'), ('map3D', 'map2D')):
        assert np.array_equal(l['host'], Z[k + idx]) and np.array_equal(l['ids'].cpu().numpy(), Z[k + idx])
        spec = dict(ids=l['host'], len=len(l['host']), members=l['members'].cpu().numpy(), offsets=l['offsets'].cpu().numpy(),
                    present=np.isin(np.arange(10), l['present']).astype(np.int32))
        assert P.map_of(spec, P.FILE_CLS) == P.recorded_map(k + m)


def test_one_epoch_of_batch_visits_every_kept_frustum_once(rt, fixture_lists):
    """SEMI_SAMPLING_METHOD BATCH at B = 1 (the smallest batch the sampler takes) over one full epoch."""
    ds, k, B = fixture_lists, P.semi_key(0.5, 0.25), 1
    idx3, idx2 = Z[k + 'idx_3Dl'], Z[k + 'idx_2Dl']
    steps = ds.partition(0, 1, B)
    assert steps == (len(idx3) + len(idx2)) // B
    ds.shuffle(5)
    s = T.Sampler(rt, ds, 'BATCH', batch=B)
    out = [s(step) for step in range(steps)]
    ids, flags = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    assert np.isin(ids[flags == 0], idx3).all() and sorted(ids[flags == 0].tolist()) == idx3.tolist()       # each exactly once
    assert np.isin(ids[flags == 1], idx2).all() and sorted(ids[flags == 1].tolist()) == idx2.tolist()
    ds.walk_len = None


def test_alternate_batch_with_equal_classes_only_names_kept_frustums(rt, fixture_lists):
    ds, k = fixture_lists, P.semi_key(0.5, 0.25)
    idx3 = Z[k + 'idx_3Dl']
    dropped = np.setdiff1d(np.nonzero(np.isin(P.FILE_CLS, TRAIN_IDS))[0], idx3)
    assert len(dropped) and not np.isin(ds.semi[0]['members'].cpu().numpy(), dropped).any()
    assert sorted(ds.semi[0]['members'].cpu().tolist()) == idx3.tolist()
    s = T.Sampler(rt, ds, 'ALTERNATE_BATCH', batch=8, prob=1.0, seed=4)
    seen = set()
    for step in range(1, 40, 2):                                                 # odd steps draw the 3-D list
        ids, flags = s(step)
        assert not flags.any() and np.isin(ids, idx3).all()
        seen |= set(ids.tolist())
    assert len(seen) > len(idx3) // 2


# ---- drivers ---------------------------------------------------------------------------------------------------------------------
class AssemblyRecorder:
    """Stands in front of the HIP library: keeps, of every t3d_batch_assemble call (made once, while the step is captured), where the
    launch reads its frustum ids -- the address and `sample_len` really placed in the argument struct."""

    def __init__(self, lib):
        self._lib, self.assemblies = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != 't3d_batch_assemble':
            return fn

        def call(a, stream):
            p = a._obj if hasattr(a, '_obj') else a.contents
            self.assemblies.append(dict(sample=C.cast(p.sample, C.c_void_p).value, sample_len=int(p.sample_len), B=int(p.B),
                                        sample2=C.cast(p.sample2, C.c_void_p).value, one_hot=C.cast(p.one_hot, C.c_void_p).value))
            return fn(a, stream)
        return call


def device_words(rt, addr, dtype):
    """(tensor, first element) of the runtime's tensor of `dtype` that holds device address `addr`."""
    holder = [t for t in rt.allocs if t.dtype == dtype and t.is_contiguous() and t.data_ptr() <= addr < t.data_ptr() + 4 * t.numel()]
    assert holder, 'the launch uses memory the runtime does not hold'
    return holder[0].view(-1), (addr - holder[0].data_ptr()) // 4


def assembled_ids(rt, rec, step):
    """The frustum id of every slot of the step that just ran, read from the device memory the assembly launch read: the slot tensor a
    sampler wrote (sample_len = 0) or perm[(step * B + b) % sample_len] (k_batch_assemble's walk)."""
    a = rec.assemblies[-1]               # (a run with other fetches may compile a plan of its own: the launch recorded last is the one that ran)
    assert a['sample2'] is None
    t, first = device_words(rt, a['sample'], torch.int32)
    if a['sample_len'] == 0:
        return t[first:first + a['B']].cpu().numpy().copy()
    # the walk may index any of sample_len entries behind the pointer: all of them must lie inside the tensor
    assert first + a['sample_len'] <= t.numel()
    walk = t[first:first + a['sample_len']].cpu().numpy()
    return walk[(step * a['B'] + np.arange(a['B'])) % a['sample_len']]


def assembled_one_hot(rt, rec):
    """The [B, 10] one-hot class rows the assembly launch wrote."""
    a = rec.assemblies[-1]
    t, first = device_words(rt, a['one_hot'], torch.float32)
    return t[first:first + a['B'] * 10].cpu().numpy().reshape(a['B'], 10)


@pytest.mark.parametrize('method', ['SAMPLE', 'BATCH'])
def test_train_boxpc_drops_frustums_of_the_2d_classes(method, hip_lib, tmp_path, monkeypatch):
    """Two steps of `train_boxpc --frustum_file <fixture> --classes_to_drop_prob 0.5`: the id of every frustum the assembly launch
    took, read back after each step, lies in the reference's idx_l -- under the class-balanced sampler (the default) and under the
    epoch permutation (BOXPC_SAMPLING_METHOD BATCH)."""
    from transferable3d_amd import api
    rec = AssemblyRecorder(hip_lib)
    rt = Runtime(lib=rec)
    steps = []
    run = api.Session.run

    def run_and_read(self, fetches, feed_dict=None):
        step = int(self.g.engine.hyper[0].item())          # the step counter the launches of this run read
        out = run(self, fetches, feed_dict)
        torch.cuda.synchronize()
        steps.append((step, assembled_ids(rt, rec, step)))
        return out
    monkeypatch.setattr(api.Session, 'run', run_and_read)
    logs = []
    flags = train_boxpc.build_flags(['--BOX_PC_MASK_REPRESENTATION', 'A', '--num_point', '256', '--batch_size', '8', '--num_channels', '4',
                                     '--max_epoch', '1', '--steps_per_epoch', '2', '--log_dir', str(tmp_path), '--frustum_file', P.FIXTURE,
                                     '--classes_to_drop_prob', '0.5', '--BOXPC_SAMPLING_METHOD', method])
    _, loss = train_boxpc.train(flags, rt=rt, log=logs.append)
    kept = Z['boxpc/drop0.5/idx_l']
    assert np.isfinite(loss) and 'Length of Train Dataset: %d' % len(kept) in logs
    assert len(rec.assemblies) >= 1 and len(steps) == 2 and [s for s, _ in steps] == [0, 1]
    assert all((a['sample_len'] == 0) == (method == 'SAMPLE') for a in rec.assemblies)
    for step, ids in steps:
        print('step %d assembled frustums %s' % (step, ids.tolist()))
        assert len(ids) == 8 and np.isin(ids, kept).all(), (method, step, ids)
    if method == 'BATCH':                                  # the walk covers whole batches of the kept frustums only, none twice
        assert all(a['sample_len'] == 16 for a in rec.assemblies) and len(set(np.concatenate([i for _, i in steps]).tolist())) == 16
    # and the class rows the launch wrote in the last step are the classes of the frustums read back
    assert np.array_equal(np.argmax(assembled_one_hot(rt, rec), 1), P.FILE_CLS[steps[-1][1]])


def _stage_a(hip_lib, tmp_path, argv, steps):
    logs = []
    flags = train_semisup.build_flags(['--SEMI_MODEL', 'A', '--WEAK_WEIGHT_REPROJECTION', '0', '--WEAK_WEIGHT_SURFACE', '0', '--num_point', '256',
                                       '--batch_size', '8', '--num_channels', '4', '--max_epoch', '1', '--steps_per_epoch', str(steps),
                                       '--frustum_file', P.FIXTURE, '--log_dir', str(tmp_path)] + argv)
    final, loss = train_semisup.train(flags, rt=Runtime(lib=hip_lib), log=logs.append)
    return final, loss, logs


def test_train_semisup_honours_the_keep_probability(hip_lib, tmp_path):
    _, loss, logs = _stage_a(hip_lib, tmp_path, ['--train_data3D_keep_prob', '0.5'], 2)
    k = P.semi_key(0.5, -1)
    assert np.isfinite(loss) and 'Length of Train Dataset: (2D: %d, 3D: %d)' % (len(Z[k + 'idx_2Dl']), len(Z[k + 'idx_3Dl'])) in logs
    # the flags at their defaults: the first step is the one of a command line without them, bit for bit
    a, loss_a, logs_a = _stage_a(hip_lib, tmp_path, ['--train_data3D_keep_prob', '1', '--add3D_for_classes2D_prob', '-1'], 1)
    b, loss_b, logs_b = _stage_a(hip_lib, tmp_path, [], 1)
    k = P.semi_key(1, -1)
    assert 'Length of Train Dataset: (2D: %d, 3D: %d)' % (len(Z[k + 'idx_2Dl']), len(Z[k + 'idx_3Dl'])) in logs_b
    print('first-step loss with the default flags %r, without %r' % (loss_a, loss_b))
    assert np.float64(loss_a).tobytes() == np.float64(loss_b).tobytes()
    assert all(np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes() for n in b)
