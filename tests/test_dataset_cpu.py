"""Device-side batch assembly (t3d_batch_assemble): the NumPy specification against the oracle's restatement of the
reference's get_classes3D / get_batch on identical draws, the statistics of the generated draws, and (below) the kernel-level
cases that tests/test_dataset_gpu.py runs on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from fake_t3d import FakeLib
from oracle import ref_data as D
from transferable3d_amd.dataset import DeviceFrustumSet, synthetic_frustums
from transferable3d_amd.engine import Runtime
from transferable3d_amd.nets import Graph, Inputs


def assemble(rt, host, B, N, Cc, sample=None, choice=None, aug=None, step=0, seed=7, **kw):
    g = Graph(B, N, Cc, rt=rt)
    x = Inputs(g)
    ds = DeviceFrustumSet(rt, **host)
    dev = rt.device
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
    g.hyper[0] = step
    a = ds.assemble_args(x, g.hyper, B, N, Cc, seed=seed, sample=t(sample, torch.int32), choice=t(choice, torch.int32),
                         aug=t(aug, torch.float32), **kw)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if dev.type == 'cuda' else None
    assert rt.lib.t3d_batch_assemble(C.byref(a), stream) == 0
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    num = lambda v: v.detach().cpu().numpy()
    pc = num(x.pc).reshape(B, N, -1)
    assert not pc[:, :, Cc:].any()                      # rows padded to 16 bytes; the padding is written as zeros
    return {'pc': pc[:, :, :Cc], 'y_seg': num(x.y_seg).reshape(B, N), 'y_center': num(x.y_center),
            'y_orient_cls': num(x.y_orient_cls), 'y_orient_reg': num(x.y_orient_reg), 'y_dims_cls': num(x.y_dims_cls),
            'y_dims_reg': num(x.y_dims_reg), 'one_hot_vec': num(x.one_hot_vec)}, ds


def check_against_oracle(rt, flags=(True, True, True)):
    B, N, Cc = 6, 256, 4
    host = synthetic_frustums(20, num_channel=6, seed=3, min_points=50, max_points=400)
    r = np.random.RandomState(1)
    sample = r.randint(0, 20, size=B)
    counts = (host['offsets'][1:] - host['offsets'][:-1])[sample]
    choice = np.stack([r.randint(0, c, size=N) for c in counts])
    flip, rn, hu = (r.uniform(size=B) > 0.5), r.normal(size=B), r.uniform(size=B)
    kw = dict(rotate_to_center=flags[0], random_flip=flags[1], random_shift=flags[2])
    got, _ = assemble(rt, host, B, N, Cc, sample=sample, choice=choice, aug=np.stack([flip, rn, hu], 1), **kw)
    compare_with_oracle(got, D.get_batch(host, sample, choice, flip, rn, hu, Cc, **kw))


def compare_with_oracle(got, ref):
    assert np.abs(got['pc'] - ref['pc']).max() < 2e-5
    assert np.array_equal(got['y_seg'], ref['y_seg'])
    assert np.abs(got['y_center'] - ref['y_center']).max() < 2e-5
    assert np.abs(got['y_dims_reg'] - ref['y_dims_reg']).max() < 1e-6 and np.array_equal(got['y_dims_cls'], ref['y_dims_cls'])
    assert np.array_equal(got['one_hot_vec'], ref['one_hot_vec'])
    # heading: class*bin + residual reproduces the angle even where fp32 puts a boundary case in the neighbouring bin
    per = 2 * np.pi / 12
    ang = lambda c, rr: (c * per + rr) % (2 * np.pi)
    d = np.abs(ang(got['y_orient_cls'], got['y_orient_reg']) - ang(ref['y_orient_cls'], ref['y_orient_reg']))
    assert np.minimum(d, 2 * np.pi - d).max() < 1e-5
    assert (got['y_orient_cls'] == ref['y_orient_cls']).mean() >= 0.8 and np.abs(got['y_orient_reg']).max() <= per / 2 + 1e-5


def check_generated_draws(rt):
    """No explicit draws: the batch follows the epoch permutation by the step counter; resampling indices are uniform over
    each frustum's points, flips come up about half the time, the z shift is within the reference's clip bounds."""
    B, N, Cc = 32, 1024, 4
    host = synthetic_frustums(100, num_channel=6, seed=5, min_points=200, max_points=900)
    got0, ds = assemble(rt, host, B, N, Cc, step=0)
    got0b, _ = assemble(rt, host, B, N, Cc, step=0)
    got1, _ = assemble(rt, host, B, N, Cc, step=1)
    assert np.array_equal(got0['pc'], got0b['pc'])                       # a function of (seed, step) only
    assert not np.array_equal(got0['pc'], got1['pc'])
    # slot b of step s holds frustum perm[(s*B + b) % F] (identity permutation here): its class id is the label
    assert np.array_equal(got0['y_dims_cls'], host['cls'][:B]) and np.array_equal(got1['y_dims_cls'], host['cls'][B:2 * B])
    # every drawn point is a point of the right frustum: the intensity channel (untouched by the augmentation) must occur there
    for b in (0, 7, 31):
        lo, hi = host['offsets'][b], host['offsets'][b + 1]
        assert np.isin(got0['pc'][b, :, 3], host['points'][lo:hi, 3]).all()
        frac_distinct = len(np.unique(got0['pc'][b, :, 3])) / min(N, hi - lo)
        assert frac_distinct > 0.55                                      # with-replacement sampling covers ~63 % when N = count
    # per-frustum statistics over many steps: flip rate and shift bounds
    flips, ok = [], True
    for step in range(2, 8):
        g, _ = assemble(rt, host, B, N, Cc, step=step)
        nf, _ = assemble(rt, host, B, N, Cc, step=step, random_flip=False, random_shift=False)
        flips.extend(np.sign(g['y_center'][:, 0]) != np.sign(nf['y_center'][:, 0]))
        dist = np.sqrt(nf['y_center'][:, 0] ** 2 + nf['y_center'][:, 1] ** 2)     # of the centre before the shifts
        shift = g['y_center'][:, 2] - nf['y_center'][:, 2]
        ok &= bool(((shift >= 0.8 * dist - 1e-4) & (shift <= 1.2 * dist + 1e-4)).all())
        assert np.abs((g['y_center'][:, 1] - nf['y_center'][:, 1])).max() <= 0.2 + 1e-5
    assert 0.3 < np.mean(flips) < 0.7 and ok


def test_batch_assembly_matches_the_reference_restatement():
    for flags in ((True, True, True), (False, False, False), (True, False, True)):
        check_against_oracle(Runtime(device='cpu', lib=FakeLib()), flags)


def test_generated_draws_and_permutation_walk():
    check_generated_draws(Runtime(device='cpu', lib=FakeLib()))


def check_alternate_batch(rt):
    """ALTERNATE_BATCH: even steps are pure weak (2-D-label classes, is_data_2D = 1), odd steps pure strong batches; a batch
    holds distinct frustums (the reference samples without replacement within a batch)."""
    B, N, Cc = 8, 128, 4
    host = synthetic_frustums(120, num_channel=6, seed=2, min_points=64, max_points=200)
    weak_cls = (1, 2, 6, 7, 8)
    g = Graph(B, N, Cc, rt=rt)
    x = Inputs(g)
    ds = DeviceFrustumSet(rt, **host).split_by_class(weak_cls)
    ds.shuffle(5)
    a = ds.assemble_args(x, g.hyper, B, N, Cc, seed=1, alternate=True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if rt.device.type == 'cuda' else None
    seen = {0: [], 1: []}
    for step in range(6):
        g.hyper[0] = step
        assert rt.lib.t3d_batch_assemble(C.byref(a), stream) == 0
        if rt.device.type == 'cuda':
            torch.cuda.synchronize()
        cls, is2d = x.one_hot_vec.cpu().numpy().argmax(1), x.is_data_2D.cpu().numpy()
        weak = step % 2 == 0
        assert (is2d == (1 if weak else 0)).all()
        assert np.isin(cls, weak_cls).all() if weak else (~np.isin(cls, weak_cls)).all()
        # a weak batch carries no 3-D label at all (get_classes2D returns zeros), a strong batch does
        lab = [x.y_seg, x.y_center, x.y_orient_cls, x.y_orient_reg, x.y_dims_cls, x.y_dims_reg]
        assert all(not bool(t.cpu().numpy().any()) for t in lab) if weak else all(bool(t.cpu().numpy().any()) for t in lab)
        key = x.pc.cpu().numpy().reshape(B, N, -1)[:, :, :3].mean(1).round(4)        # distinct frustums -> distinct point clouds
        assert len(np.unique(key, axis=0)) == B
        seen[step % 2].append(cls.copy())
    assert not np.array_equal(seen[0][0], seen[0][1])               # the lists advance


def test_alternate_batch_sampling():
    check_alternate_batch(Runtime(device='cpu', lib=FakeLib()))


def _stream(lib_is_fake):
    if lib_is_fake:
        return None
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _perturb_inputs(r, B):
    return dict(center=(r.normal(size=(B, 3)) * 0.3 + [0, 0, 3]).astype(np.float32), ocls=r.randint(0, 12, B).astype(np.int32),
                oreg=(r.uniform(-1, 1, B) * np.pi / 12).astype(np.float32), cls=r.randint(0, 10, B).astype(np.int32),
                dreg=(r.normal(size=(B, 3)) * 0.1).astype(np.float32))


def run_perturb(lib, dev, base, B, rounds, fit_u=None, cand=None, step=0, seed=77):
    from transferable3d_amd import abi
    from transferable3d_amd.abi import fptr, iptr
    t = {k: torch.as_tensor(v.copy()).to(dev) for k, v in base.items()}
    o = dict(iou=torch.zeros(B, device=dev), dc=torch.zeros(B, 3, device=dev), ds=torch.zeros(B, 3, device=dev), da=torch.zeros(B, device=dev))
    hyper = torch.tensor([float(step), 0, 0, 0], device=dev)
    fu = torch.as_tensor(fit_u).to(dev) if fit_u is not None else None
    cd = torch.as_tensor(cand).to(dev) if cand is not None else None
    a = abi.BoxPcPerturbArgs(fptr(t['center']), iptr(t['ocls']), fptr(t['oreg']), iptr(t['cls']), fptr(t['dreg']), fptr(o['iou']), fptr(o['dc']),
                             fptr(o['ds']), fptr(o['da']), 0.8, 0.2, np.pi, 0.7, 1.0, 0.01, 0.25, 0.5, fptr(fu), fptr(cd), rounds, seed, fptr(hyper), B)
    assert lib.t3d_boxpc_perturb(C.byref(a), _stream(isinstance(lib, FakeLib))) == 0
    if dev != 'cpu':
        torch.cuda.synchronize()
    return {k: v.cpu() for k, v in t.items()}, {k: v.cpu() for k, v in o.items()}


def check_boxpc_perturb_against_oracle(lib, dev):
    """t3d_boxpc_perturb (first accepted candidate of a 64-wide candidate stream) against the oracle's restatement of
    BoxPCFitDataset.perturb_box_to_diff_ious (sequential rejection sampling) consuming the same uniforms."""
    from oracle import ref_data as RD
    from transferable3d_amd.constants import MEAN_DIMS_ARR
    r = np.random.RandomState(4)
    B, R = 24, 6
    base = _perturb_inputs(r, B)
    fit_u = r.uniform(size=B).astype(np.float32)
    cand = r.uniform(size=(B, R * 64, 7)).astype(np.float32)
    t, o = run_perturb(lib, dev, base, B, R, fit_u, cand)
    n_fit = 0
    for b in range(B):
        heading = base['ocls'][b] * (2 * np.pi / 12) + float(base['oreg'][b])
        size = MEAN_DIMS_ARR[base['cls'][b]] + base['dreg'][b].astype(np.float64)
        is_fit = fit_u[b] < 0.5
        n_fit += is_fit
        want = RD.boxpc_sample_labels(base['center'][b].astype(np.float64), heading, size, int(base['cls'][b]), is_fit, (0.7, 1.0), (0.01, 0.25),
                                      (0.8, 0.2, np.pi), cand[b].astype(np.float64))
        assert want is not None, b
        lo, hi = ((0.7, 1.0) if is_fit else (0.01, 0.25))
        assert lo < float(o['iou'][b]) < hi
        assert abs(float(o['iou'][b]) - want['y_box_iou']) < 2e-5
        assert np.abs(t['center'][b].numpy() - want['x_center']).max() < 1e-5
        assert int(t['ocls'][b]) == want['x_orient_cls'] and abs(float(t['oreg'][b]) - want['x_orient_reg']) < 1e-5
        assert np.abs(t['dreg'][b].numpy() - want['x_dims_reg']).max() < 1e-5
        assert np.abs(o['dc'][b].numpy() - want['y_center_delta']).max() < 1e-6
        assert np.abs(o['ds'][b].numpy() - want['y_dims_delta']).max() < 1e-6
        assert abs(float(o['da'][b]) - want['y_orient_delta']) < 1e-6
    assert 0 < n_fit < B


def check_boxpc_perturb_generated(lib, dev):
    """Generated draws (hash of seed, step, frustum, candidate): every sample lands inside its bounds, about half are "fit", the
    deltas reproduce the perturbed box, and a different step gives different samples."""
    from fake_t3d import box3d_iou_spec
    from transferable3d_amd.constants import MEAN_DIMS_ARR
    B = 64
    base = _perturb_inputs(np.random.RandomState(9), B)
    t, o = run_perturb(lib, dev, base, B, 4, step=3)
    iou = o['iou'].numpy()
    fit = iou > 0.7
    assert np.all(((iou > 0.7) & (iou < 1.0)) | ((iou > 0.01) & (iou < 0.25))) and 16 < fit.sum() < 48
    for b in range(0, B, 7):
        h0 = base['ocls'][b] * (2 * np.pi / 12) + base['oreg'][b]
        s0 = MEAN_DIMS_ARR[base['cls'][b]] + base['dreg'][b]
        h1 = int(t['ocls'][b]) * (2 * np.pi / 12) + float(t['oreg'][b])
        s1 = MEAN_DIMS_ARR[base['cls'][b]] + t['dreg'][b].numpy()
        assert np.abs(t['center'][b].numpy() - base['center'][b] - o['dc'][b].numpy()).max() < 1e-6
        assert np.abs(s1 - s0 - o['ds'][b].numpy()).max() < 1e-6
        assert abs(np.angle(np.exp(1j * (h1 - h0 - float(o['da'][b]))))) < 1e-5
        assert abs(box3d_iou_spec(base['center'][b], s0, h0, t['center'][b].numpy(), s1, h1)[0] - iou[b]) < 2e-5
    _, o2 = run_perturb(lib, dev, base, B, 4, step=4)
    assert not np.allclose(o2['iou'].numpy(), iou)
    return base, t, o


def test_boxpc_perturb_spec_against_oracle_on_identical_draws():
    check_boxpc_perturb_against_oracle(FakeLib(), 'cpu')


def test_boxpc_perturb_generated_draws_follow_the_sampling_law():
    check_boxpc_perturb_generated(FakeLib(), 'cpu')


def test_frustum_pickle_reader(tmp_path):
    """A file in the reference's format -- gzip'd protocol-2 pickle of the 13 lists, class names as Python-2 byte strings -- loads
    into a DeviceFrustumSet: ragged point lists, box centre = (corner0 + corner6) / 2, class filter."""
    import gzip
    import pickle
    from transferable3d_amd.dataset import load_zipped_pickle
    r = np.random.RandomState(2)
    names = [b'bed', b'chair', b'table', b'chair', b'sofa']
    n = [300, 120, 77, 500, 64]
    box3d = [r.normal(size=(8, 3)) for _ in names]
    lists = [list(range(5)), [r.uniform(size=4) for _ in names], box3d, [None] * 5, [r.normal(size=(k, 6)) for k in n],
             [(r.uniform(size=k) < 0.3).astype(np.float64) for k in n], names, list(r.uniform(-3, 3, 5)), [r.uniform(0.5, 2, 3) for _ in names],
             [np.eye(3)] * 5, [np.eye(3)] * 5, list(r.uniform(-2, -1, 5)), [np.array([640, 480])] * 5]
    path = str(tmp_path / 'train_mini.zip.pickle')
    with gzip.open(path, 'wb') as f:
        pickle.dump(lists, f, 2)
    back = load_zipped_pickle(path)
    assert back[6] == ['bed', 'chair', 'table', 'chair', 'sofa'] and np.array_equal(back[4][2], lists[4][2])
    rt = Runtime(device='cpu', lib=FakeLib())
    ds = DeviceFrustumSet.from_pickle(rt, path, classes=['chair', 'sofa'])
    assert ds.F == 3 and ds.image_ids == [1, 3, 4]
    assert ds.offsets.tolist() == [0, 120, 620, 684] and ds.cls.tolist() == [3, 3, 2]
    assert np.allclose(ds.box_center[1].numpy(), (box3d[3][0] + box3d[3][6]) / 2, atol=1e-6)
    assert np.allclose(ds.points[120:620].numpy(), lists[4][3].astype(np.float32)) and ds.seg[620:].tolist() == lists[5][4].astype(int).tolist()
    all_ds = DeviceFrustumSet.from_pickle(rt, path)
    assert all_ds.F == 5


def run_equal_sampler(lib, dev, ds, B, step, seed=5, alternate=False, equal_prob=1.0, order=None, member=None, prob=None):
    hyper = torch.tensor([float(step), 0, 0, 0], device=dev)
    out = torch.zeros(B, dtype=torch.int32, device=dev)
    flag = torch.full((B,), -1, dtype=torch.int32, device=dev)
    mk = lambda v: None if v is None else torch.as_tensor(np.asarray(v, np.float32)).to(dev)
    a = ds.sample_equal_args(hyper, B, out, is_data_2D=flag, seed=seed, equal_prob=equal_prob, alternate=alternate, order_draws=mk(order),
                             member_draws=mk(member), prob_draw=mk(prob))
    assert lib.t3d_sample_equal_classes(C.byref(a), _stream(isinstance(lib, FakeLib))) == 0
    if dev != 'cpu':
        torch.cuda.synchronize()
    return out.cpu().numpy(), flag.cpu().numpy()


def check_equal_class_sampler(rt):
    """t3d_sample_equal_classes against the oracle's restatement of `equal_samples_per_class` on identical draws, the law of the
    generated draws, the two-list (ALTERNATE_BATCH) mode and the not-balanced fallback."""
    lib, dev = rt.lib, rt.device.type if rt.device.type == 'cpu' else 'cuda'
    host = synthetic_frustums(120, num_channel=4, seed=3, min_points=130, max_points=200)
    ds = DeviceFrustumSet(rt, **host)
    cls = host['cls']
    present = sorted(set(int(c) for c in cls))
    lists = [np.nonzero(cls == c)[0] for c in present]
    n = len(present)
    r = np.random.RandomState(1)
    for B in (32, 7, 60):
        order, member = r.uniform(size=n).astype(np.float32), r.uniform(size=B).astype(np.float32)
        got, flag = run_equal_sampler(lib, dev, ds, B, step=3, order=order, member=member)
        # the oracle's shuffled np.array_split: the `B % n` groups with the smallest keys are the larger ones
        rank = np.argsort(np.argsort(order, kind='stable'), kind='stable')
        split = [np.ones(B // n + (1 if rank[i] < B % n else 0)) for i in range(n)]
        assert sorted(len(s) for s in split) == sorted(len(s) for s in np.array_split([1] * B, n))
        want = D.sample_equal_per_class(B, lists, split, member.astype(np.float64))
        assert got.tolist() == [int(w) for w in want] and (flag == 0).all()
    # generated draws: every class gets floor(B/n) or ceil(B/n) slots, slots grouped by class, different steps differ
    B = 32
    a, _ = run_equal_sampler(lib, dev, ds, B, step=10)
    b, _ = run_equal_sampler(lib, dev, ds, B, step=11)
    counts = np.bincount(cls[a], minlength=10)[present]
    assert counts.min() >= B // n and counts.max() <= B // n + 1 and (np.diff(cls[a]) >= 0).all()
    assert not np.array_equal(a, b)
    # over many steps every frustum of a class is drawn about equally often
    hits = np.zeros(len(cls))
    for s in range(200):
        np.add.at(hits, run_equal_sampler(lib, dev, ds, B, step=s)[0], 1)
    per_class = [hits[l] / hits[l].sum() for l in lists]
    assert all(np.abs(p - 1.0 / len(p)).max() < 4.0 / np.sqrt(200 * B / n) / np.sqrt(len(p)) + 0.05 for p in per_class)
    # two lists: even steps from the weak (2-D label) classes with is_data_2D = 1, odd steps from the others with 0
    weak_ids = [1, 2, 6, 7, 8]
    ds.split_by_class(weak_ids)
    e, fe = run_equal_sampler(lib, dev, ds, B, step=4, alternate=True)
    o, fo = run_equal_sampler(lib, dev, ds, B, step=5, alternate=True)
    assert np.isin(cls[e], weak_ids).all() and (fe == 1).all() and (~np.isin(cls[o], weak_ids)).all() and (fo == 0).all()
    # equal_prob = 0: the next B entries of the epoch permutation (B distinct frustums)
    p0, _ = run_equal_sampler(lib, dev, DeviceFrustumSet(rt, **host), B, step=2, equal_prob=0.0)
    ds2 = DeviceFrustumSet(rt, **host)
    p1, _ = run_equal_sampler(lib, dev, ds2, B, step=2, equal_prob=0.0)
    assert np.array_equal(p0, p1) and len(set(p1.tolist())) == B and np.array_equal(p1, ds2.perm.cpu().numpy()[2 * B:3 * B])
    # a draw above equal_prob takes the permutation, below it the balanced composition
    hi, _ = run_equal_sampler(lib, dev, ds2, B, step=2, equal_prob=0.5, prob=[0.7])
    lo, _ = run_equal_sampler(lib, dev, ds2, B, step=2, equal_prob=0.5, prob=[0.3])
    assert np.array_equal(hi, p1) and (np.diff(cls[lo]) >= 0).all()


def test_equal_samples_per_class_sampler():
    check_equal_class_sampler(Runtime(device='cpu', lib=FakeLib()))


def test_combined_data_set_marks_two_d_frustums():
    """SEMI_SAMPLING_METHOD BATCH: is_data_2D follows the per-frustum flag of the combined data set."""
    rt = Runtime(device='cpu', lib=FakeLib())
    host = synthetic_frustums(40, num_channel=4, seed=6, min_points=130, max_points=160)
    ds = DeviceFrustumSet(rt, **host).mark_2d_classes([1, 2, 6, 7, 8])
    B, N, Cc = 8, 128, 4
    g = Graph(B, N, Cc, rt=rt)
    x = Inputs(g)
    g.hyper[0] = 2.0
    a = ds.assemble_args(x, g.hyper, B, N, Cc, seed=3)
    assert rt.lib.t3d_batch_assemble(C.byref(a), None) == 0
    f = ds.perm.numpy()[2 * B:3 * B]
    assert np.array_equal(x.is_data_2D.numpy(), np.isin(host['cls'][f], [1, 2, 6, 7, 8]).astype(np.int32))
    assert 0 < x.is_data_2D.sum() < B


def test_epoch_is_one_pass_and_replicas_walk_disjoint_slices():
    """train_semisup.py:330-349: an epoch visits every frustum once (whole batches; the remainder is dropped as in the reference);
    data-parallel replicas share the epoch permutation and take disjoint slices of it; the device-side walk position
    (step * B + b) % walk_len stays aligned with the epoch boundaries."""
    from fake_t3d import FakeLib
    from transferable3d_amd.dataset import DeviceFrustumSet
    from transferable3d_amd.engine import Runtime
    F, B, world = 50, 4, 2
    seen = []
    for rank in range(world):
        ds = DeviceFrustumSet.synthetic(Runtime(device='cpu', lib=FakeLib()), F, 4, seed=1, min_points=8, max_points=16)
        steps = ds.partition(rank, world, B)
        assert steps == (F // world) // B == 6 and ds.walk_len == 24
        per_epoch = []
        for epoch in range(2):
            ds.shuffle(1000 + epoch)                  # the same seed on every replica
            perm = ds.perm.numpy()
            walk = [int(perm[((epoch * steps + s) * B + b) % ds.walk_len]) for s in range(steps) for b in range(B)]
            assert len(set(walk)) == len(walk) == 24          # nothing repeated inside a pass
            per_epoch.append(set(walk))
        seen.append(per_epoch)
        assert ds.partition(rank, world, B, steps=3) == 3 and ds.walk_len == 12
    for epoch in range(2):
        assert not (seen[0][epoch] & seen[1][epoch])           # replicas see disjoint frustums
        assert len(seen[0][epoch] | seen[1][epoch]) == 48      # 50 frustums, 2 dropped with the incomplete batch


# ---- t3d_batch_assemble at kernel level: a direct call on guarded operands (tests/guard_bands.py), at the shapes the data-set wrapper
# and the comfortable frustums of the checks above never reach ----

EDGE_COUNTS = (1, 5, 64, 65, 1)              # the 1-point frustum is the set's first and its last; 64 / 65: a wave and one more
LAYOUTS = ((6, 3, 4), (6, 4, 4), (6, 6, 8), (4, 4, 0))          # (C_src, C, ld_pc)


def edge_set(C_src, counts=EDGE_COUNTS, seed=0, heading=None):
    """A tiny ragged set of fp32-exact values; channel 3 (where there is one) holds the point's row in `points`, so that a copied
    channel names the row a draw took."""
    r = np.random.RandomState(seed)
    F, total = len(counts), int(np.sum(counts))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    pts = (r.normal(size=(total, C_src)) * 0.5 + np.array([0, 0, 3] + [0] * (C_src - 3))).astype(np.float32)
    if C_src > 3:
        pts[:, 3] = np.arange(total)
    return dict(points=pts, seg=r.randint(0, 2, total).astype(np.int32), offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                frustum_angle=f32(r.uniform(-0.6, 0.6, F) - np.pi / 2), box_center=f32(r.normal(size=(F, 3)) * 0.2 + [0, 0.2, 3]),
                heading=f32(r.uniform(-np.pi, np.pi, F) if heading is None else heading), size=f32(r.uniform(0.5, 2, (F, 3))),
                cls=r.randint(0, 10, F).astype(np.int32))


def assemble_direct(lib, dev, host, B, N, Cc, ld_pc=0, sample=None, sample_len=0, choice=None, aug=None, step=0, seed=7,
                    rotate_to_center=True, random_flip=True, random_shift=True):
    """One t3d_batch_assemble call with every operand in guard bands: a NaN / INT_BAND row stands right behind the last frustum of
    `points` / `seg`.  Checks that the inputs are unchanged, that nothing is stored outside the outputs, that every output element
    (the pad columns of pc included: zeros) is written and that pc is finite; returns the outputs."""
    from guard_bands import guarded
    from transferable3d_amd import abi
    from transferable3d_amd.abi import fptr, iptr
    F32, I32 = torch.float32, torch.int32
    F = len(host['cls'])
    ins = dict(points=(host['points'], F32), seg=(host['seg'], I32), offsets=(host['offsets'], torch.int64),
               frustum_angle=(host['frustum_angle'], F32), box_center=(host['box_center'], F32), heading=(host['heading'], F32),
               size=(host['size'], F32), cls=(host['cls'], I32), sample=(np.asarray(sample), I32),
               hyper=(np.array([step, 0, 0, 0], np.float32), F32))
    if choice is not None:
        ins['choice'] = (np.asarray(choice), I32)
    if aug is not None:
        ins['aug'] = (np.asarray(aug), F32)
    ld = ld_pc or Cc
    outs = dict(pc=((B * N, ld), F32), y_seg=((B, N), I32), y_center=((B, 3), F32), y_orient_cls=((B,), I32), y_orient_reg=((B,), F32),
                y_dims_cls=((B,), I32), y_dims_reg=((B, 3), F32), one_hot=((B, 10), F32), rot_angle=((B,), F32), is_data_2D=((B,), I32))
    t, chk = {}, {}
    for k, (a, dt) in ins.items():
        t[k], chk[k] = guarded(np.shape(a), dt, dev, fill=torch.as_tensor(np.ascontiguousarray(a)), name=k)
    for k, (shape, dt) in outs.items():
        t[k], chk[k] = guarded(shape, dt, dev, name=k)
    a = abi.BatchAssembleArgs()
    for k in t:
        ptr = abi.C.cast(abi.C.c_void_p(t[k].data_ptr()), abi.C.POINTER(abi.C.c_int64)) if k == 'offsets' else \
            (fptr if t[k].dtype == F32 else iptr)(t[k])
        setattr(a, k, ptr)
    a.sample_len, a.C_src, a.C, a.B, a.N, a.ld_pc, a.seed = sample_len, host['points'].shape[1], Cc, B, N, ld_pc, seed
    a.rotate_to_center, a.random_flip, a.random_shift = int(rotate_to_center), int(random_flip), int(random_shift)
    assert lib.t3d_batch_assemble(C.byref(a), _stream(isinstance(lib, FakeLib))) == 0
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    for k, ck in chk.items():
        ck(written=True) if k in outs else ck()
    num = {k: t[k].cpu().numpy().copy() for k in outs}
    pc = num['pc'].reshape(B, N, ld)
    assert np.isfinite(pc).all() and not pc[:, :, Cc:].any()                # no band row was drawn; the pad columns are zeros
    num['pc'], num['one_hot_vec'] = pc[:, :, :Cc], num.pop('one_hot')
    return num


def check_small_frustums(lib, dev):
    """Frustums of 1, 5, 64 and 65 points, every slot sampling each of them, in every row layout.  Generated draws: 0 <= ch < cnt,
    read off the copied channel that names the source row (and, for another library than the specification, the specification's
    draws); given draws that hold 0 and cnt - 1: the oracle restatement."""
    F, N = len(EDGE_COUNTS), 300                                            # two workgroups per slot
    for C_src, Cc, ld in LAYOUTS:
        host = edge_set(C_src, seed=C_src + Cc)
        off, cnt = host['offsets'], np.asarray(EDGE_COUNTS)
        for roll in range(F):
            sample = np.roll(np.arange(F), roll)
            kw = dict(ld_pc=ld, sample=sample, step=roll, seed=11)
            gen = assemble_direct(lib, dev, host, F, N, Cc, **kw)
            if Cc > 3:
                row = gen['pc'][:, :, 3].astype(np.int64)
                ch = row - off[sample][:, None]
                assert (gen['pc'][:, :, 3] == row).all() and (ch >= 0).all() and (ch < cnt[sample][:, None]).all()
                assert np.array_equal(gen['y_seg'], host['seg'][row])
                for b in range(F):
                    if cnt[sample[b]] <= 5:
                        assert set(ch[b].tolist()) == set(range(cnt[sample[b]]))          # every point of a tiny frustum is drawn
            assert np.array_equal(gen['y_dims_cls'], host['cls'][sample]) and not gen['is_data_2D'].any()
            if not isinstance(lib, FakeLib):                                # the tolerances of test_generated_batch_equals_the_specification
                c = assemble_direct(FakeLib(), 'cpu', host, F, N, Cc, **kw)
                assert np.array_equal(c['y_seg'], gen['y_seg']) and np.array_equal(c['pc'][:, :, 3:], gen['pc'][:, :, 3:])
                assert np.abs(c['pc'] - gen['pc']).max() < 1e-4 and np.abs(c['y_center'] - gen['y_center']).max() < 1e-4
                assert np.array_equal(c['y_orient_cls'], gen['y_orient_cls']) and np.abs(c['y_orient_reg'] - gen['y_orient_reg']).max() < 1e-5
            r = np.random.RandomState(roll)
            choice = np.stack([r.randint(0, n, size=N) for n in cnt[sample]])
            choice[:, 0], choice[:, 1], choice[:, N - 1] = cnt[sample] - 1, 0, cnt[sample] - 1
            flip, rn, hu = (r.uniform(size=F) > 0.5), r.normal(size=F), r.uniform(size=F)
            got = assemble_direct(lib, dev, host, F, N, Cc, ld_pc=ld, sample=sample, choice=choice, aug=np.stack([flip, rn, hu], 1))
            compare_with_oracle(got, D.get_batch(host, sample, choice, flip, rn, hu, Cc))


def check_heading_bin_edges(lib, dev):
    """Headings exactly on the 12 bin edges, one fp32 step either side of them and further off, negative headings, and each of them
    flipped (pi - h), in one batch against the oracle restatement with the tolerances of check_against_oracle: class * bin + residual
    gives the angle back whichever bin fp32 chooses at an edge, the residual stays within half a bin, and the bins agree for
    at least 0.8 of the batch -- 36 of its 180 headings lie within an fp32 step of an edge, the others at least 1e-3 away."""
    per = 2 * np.pi / 12
    edges = np.float32(np.arange(12) * per - per / 2)
    near = np.concatenate([edges, np.nextafter(edges, np.float32(-9)), np.nextafter(edges, np.float32(9))])
    off = np.concatenate([s * (edges.astype(np.float64) + d) for s in (1, -1) for d in (1e-3, -1e-3, 0.1, -0.1, 0.2, -0.2)])
    heading = np.concatenate([near.astype(np.float64), off])
    B = len(heading)
    assert B == 180 and (heading < 0).sum() > 60
    host = edge_set(4, counts=(3,) * B, seed=3, heading=heading)
    choice = np.random.RandomState(0).randint(0, 3, size=(B, 4))
    for flipped in (False, True):
        flip = np.full(B, flipped)
        got = assemble_direct(lib, dev, host, B, 4, 4, sample=np.arange(B), choice=choice, aug=np.stack([flip, 0.0 * flip, 0.0 * flip], 1),
                              rotate_to_center=False, random_shift=False)
        ref = D.get_batch(host, np.arange(B), choice, flip, np.zeros(B), np.zeros(B), 4, rotate_to_center=False, random_shift=False)
        compare_with_oracle(got, ref)
        assert np.array_equal(got['y_orient_cls'][36:], ref['y_orient_cls'][36:])          # 1e-3 and more from an edge: fp32 resolves it
        assert set(got['y_orient_cls'].tolist()) == set(range(12))


def check_batch_of_one_and_wrapping_walk(lib, dev):
    """B = 1, and a permutation walk shorter than the batch: slot b of step s takes sample[(s * B + b) mod sample_len], the same
    bytes as naming those frustums slot by slot (the generated draws follow seed, step, slot and point, not the frustum)."""
    host = edge_set(6, seed=5)
    one = assemble_direct(lib, dev, host, 1, 70, 6, ld_pc=8, sample=[3], step=4)
    assert int(one['y_dims_cls'][0]) == host['cls'][3] and one['one_hot_vec'][0].argmax() == host['cls'][3]
    row = one['pc'][0, :, 3]
    assert (row >= host['offsets'][3]).all() and (row < host['offsets'][4]).all()
    perm, B, step = np.array([4, 0, 2], np.int32), 4, 2
    walk = assemble_direct(lib, dev, host, B, 70, 6, ld_pc=8, sample=perm, sample_len=3, step=step)
    named = perm[(step * B + np.arange(B)) % 3]
    assert named.tolist() == [2, 4, 0, 2]                                   # wraps inside the batch
    same = assemble_direct(lib, dev, host, B, 70, 6, ld_pc=8, sample=named, step=step)
    assert np.array_equal(walk['y_dims_cls'], host['cls'][named])
    for k in walk:
        assert walk[k].tobytes() == same[k].tobytes(), k


def test_small_frustums_in_every_row_layout():
    check_small_frustums(FakeLib(), 'cpu')


def test_headings_on_the_bin_edges():
    check_heading_bin_edges(FakeLib(), 'cpu')


def test_batch_of_one_and_a_walk_that_wraps_inside_the_batch():
    check_batch_of_one_and_wrapping_walk(FakeLib(), 'cpu')


def test_a_set_with_an_empty_frustum_is_refused():
    """t3d_batch_assemble would read the row behind an empty frustum (t3d.h); the set refuses it, wherever it stands, and no kernel
    is launched on one anywhere."""
    rt = Runtime(device='cpu', lib=FakeLib())
    for where, counts in ((0, (0, 5, 7)), (1, (5, 0, 7)), (2, (5, 7, 0)), (1, (4, 0, 0))):
        host = edge_set(4, counts=counts)
        with pytest.raises(ValueError, match='frustum %d of 3 holds no points' % where):
            DeviceFrustumSet(rt, **host)
        r = np.random.RandomState(0)
        lists = [r.normal(size=(n, 4)) for n in counts], [np.zeros(n) for n in counts]
        with pytest.raises(ValueError, match='frustum %d of 3 holds no points' % where):
            DeviceFrustumSet.from_lists(rt, lists[0], lists[1], host['frustum_angle'], host['box_center'], host['heading'], host['size'], host['cls'])
    out = {'out_points': torch.zeros(3, 8, 4, dtype=torch.float64), 'frustum_angle': torch.zeros(3, dtype=torch.float64)}
    with pytest.raises(ValueError, match='frustum 1 of 2 holds no points'):
        DeviceFrustumSet.from_device(rt, out, [0, 2], [5, 0], [1, 2])
    assert DeviceFrustumSet.from_device(rt, out, [0, 2], [5, 1], [1, 2]).offsets.tolist() == [0, 5, 6]
    assert DeviceFrustumSet(rt, **edge_set(4, counts=(1, 1))).F == 2
