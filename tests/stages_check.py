"""Shared body of the stage-order tests (test_detect_stages_cpu.py: NumPy specification libraries; test_detect_stages_gpu.py: libt3d.so):
one `Detector.decode_all` call that runs every stage behind t3d_detect_decode -- two views, the consistency measures with a threshold,
min_view_iou, NMS and box voting -- and what each stage was handed.

The scenes are the golden ones of detect_check.write_data_set with their image sizes; every detection but the sparse one is reported a
second time a few pixels off at half the confidence (the device of test_a_detection_rejected_by_min_view_iou_suppresses_nothing), so that
every (image, class) group holds a pair.  The second reports stand behind their scene's own detections: with each directly behind its
first report, the thresholds reject both reports of an object or neither on these scenes, and no accepted detection is left behind a
rejected better-ranked partner -- which `check_flow` asserts there is.  The two thresholds are midpoints between order statistics of a first run without thresholds on
the same runtime, so nothing here depends on a device's last bits.

`Stages` wraps DeviceEnsemble.run, DeviceNms.run, DeviceFuse.run and Renderer.render_tables (the one call of t3d_render: the corners it
hands the library lie in device memory, where the library's own entry point cannot be read from Python) and keeps host copies of what
they read and wrote; for its length the runtime's library is a proxy that lists the t3d_detect_* entry points in the order they are
called.  `CpuCalls` counts torch.Tensor.cpu, without the copies `Stages` makes."""
import contextlib

import numpy as np
import torch

import consistency_check as CC
import detect_check as DC
import ensemble_check as EC
import fake_ensemble as FE
import fake_fuse as FF
import fake_nms as FN
import fuse_check as FC
import nms_check as NC
from transferable3d_amd import detect as DT, ensemble as EN, nms as NMS, render as RD, test_semisup as TS

NMS_IOU = 0.05
SHIFT = (6.0, 4.0, 6.0, 4.0)
# Tensor.cpu calls inside decode_all for this configuration (18 detections in 5 batches of 4), read off the commit before the stages got
# one owner: consistency 2, the agreement for min_view_iou 1, the decode's two allocations 2, NMS 2, the ensemble 2 x 2 + 6, the fusion 3
CPU_CALLS = 20


class CpuCalls:
    """Counts torch.Tensor.cpu while it is entered and not paused."""

    def __init__(self):
        self.n, self.off = 0, 0

    def __enter__(self):
        self.real = torch.Tensor.cpu
        counter = self

        def cpu(t, *a, **kw):
            counter.n += not counter.off
            return counter.real(t, *a, **kw)

        torch.Tensor.cpu = cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu = self.real

    @contextlib.contextmanager
    def paused(self):
        self.off += 1
        try:
            yield
        finally:
            self.off -= 1


class LibProxy:
    """The runtime's library; every t3d_detect_* entry point called through it is listed in `names` (without the prefix)."""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith('t3d_detect_'):
            return f

        def call(*a):
            self._names.append(name[len('t3d_detect_'):])
            return f(*a)
        return call


class Stages:
    """Host copies of what the ensemble, NMS, fusion and render calls of a run read and wrote, and the order of the t3d_detect_* calls."""

    def __init__(self, rt, counter=None):
        self.rt, self.counter = rt, counter or CpuCalls()
        self.entry_points, self.ensemble, self.nms, self.fuse, self.render = [], [], [], [], []

    def host(self, t):
        with self.counter.paused():
            return None if t is None else t.detach().cpu().numpy().copy()

    def __enter__(self):
        cap, host = self, self.host
        self.real = (EN.DeviceEnsemble.run, NMS.DeviceNms.run, NMS.DeviceFuse.run, RD.Renderer.render_tables, self.rt.lib)

        def ensemble(dev, labels, weights, corners0, flip_mask=0, rot_angle=None, vote_threshold=0.0, metric='3d', fill=None):
            call = dict(labels=np.stack([host(t).reshape(-1, 7) for t in labels]), weights=np.stack([host(t).reshape(-1) for t in weights]),
                        corners0=host(corners0).reshape(-1, 8, 3), flip_mask=flip_mask, rot=host(rot_angle), vote=vote_threshold, metric=metric)
            out = cap.real[0](dev, labels, weights, corners0, flip_mask, rot_angle, vote_threshold, metric, fill)
            call['out'] = dict(zip(FE.OUTPUTS, [host(t) for t in out]))
            cap.ensemble.append(call)
            return out

        def nms(dev, corners, score, group_offsets, members, threshold, metric='3d', fill=None):
            call = dict(corners=host(corners).reshape(-1, 8, 3), score=host(score), offsets=np.array(group_offsets), members=np.array(members),
                        threshold=threshold, metric=metric)
            out = cap.real[1](dev, corners, score, group_offsets, members, threshold, metric, fill)
            call['keep'], call['suppressed_by'], call['rank'] = (host(t) for t in out)
            cap.nms.append(call)
            return out

        def fuse(dev, nms_dev, label, corners, weight, vote_threshold, fill=None):
            call = dict(label=host(label).reshape(-1, 7), corners=host(corners).reshape(-1, 8, 3), weight=host(weight), vote=vote_threshold)
            out = cap.real[2](dev, nms_dev, label, corners, weight, vote_threshold, fill)
            call['label_out'], call['corners_out'], call['n_votes'] = (host(t) for t in out)
            call['corners_out'] = call['corners_out'].reshape(-1, 8, 3)
            cap.fuse.append(call)
            return out

        def render_tables(ren, *a, **kw):
            cap.render.append(host(kw['corners']).reshape(-1, 8, 3))
            return cap.real[3](ren, *a, **kw)

        EN.DeviceEnsemble.run, NMS.DeviceNms.run, NMS.DeviceFuse.run, RD.Renderer.render_tables = ensemble, nms, fuse, render_tables
        self.rt.lib = LibProxy(self.real[4], self.entry_points)
        return self

    def __exit__(self, *exc):
        EN.DeviceEnsemble.run, NMS.DeviceNms.run, NMS.DeviceFuse.run, RD.Renderer.render_tables, self.rt.lib = self.real


def doubled(dets):
    """Behind the detections of every scene, a second report of each but the sparse one: its box a few pixels off, half its confidence."""
    return [list(scene) + [(x[0], tuple(np.asarray(x[1]) + SHIFT), x[2] / 2.0) for x in scene if x != DC.SPARSE] for scene in dets]


def between(values, k):
    """The midpoint between the values of rank k - 1 and k (from 0, ascending): exactly k of them lie below it."""
    v = np.sort(np.asarray(values, np.float64))
    assert v[k - 1] < v[k], (k, v)
    return float((v[k - 1] + v[k]) / 2.0)


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def check_flow(rt, root, exact):
    """exact: `rt` runs the specification itself; the comparisons with the specification are byte comparisons and the counts of the log
    lines and of Tensor.cpu are pinned.  Otherwise the specification is met within the bounds of ensemble_check.compare and
    fuse_check.label_bounds.  What one stage hands the next is the same device memory and is compared as bytes either way.
    -> report lines."""
    ids, folder, idx, dets = DC.write_data_set(root)
    dets = doubled(dets)
    scenes = CC.scenes_with_sizes(root, ids)
    flags = lambda: TS.build_flags(DC.MODEL_FLAGS)
    plain = [r for recs in DT.Detector(flags(), rt=rt).detect(scenes, dets, scene_ids=ids) for r in recs]
    n = len(plain)
    assert n == 18 and n == sum(len(s) for s in dets) - 1

    # ---- the thresholds, from a run without any ----------------------------------------------------------------------------------
    first = DT.Detector(flags(), rt=rt, tta=2, tta_flip=True, consistency=True)
    _, d0 = first.decode_all([first.extract(scenes, dets, ids)])
    A, M = between(d0.view_iou, n // 3), between(d0.mask_in_box, 2)

    # ---- every stage in one call -------------------------------------------------------------------------------------------------
    lines = []
    options = dict(tta=2, tta_flip=True, nms_iou=NMS_IOU, nms_fuse=True, min_view_iou=A, min_mask_in_box=M)
    det = DT.Detector(flags(), rt=rt, log=lines.append, **options)
    parts = [det.extract(scenes, dets, ids)]
    counter = CpuCalls()
    with counter, Stages(rt, counter) as cap:
        meta, d = det.decode_all(parts)
    assert len(meta) == len(d) == n
    assert [m[2] for m in meta] == [r['class'] for r in plain] and [m[4] for m in meta] == [r['prob'] for r in plain]
    batches = (n + 3) // 4
    assert cap.entry_points == ['decode', 'decode', 'consistency'] * batches + ['ensemble', 'nms', 'fuse'], cap.entry_points
    assert len(cap.ensemble) == len(cap.nms) == len(cap.fuse) == 1 and not cap.render
    ens, nms, fuse = cap.ensemble[0], cap.nms[0], cap.fuse[0]
    e = {k: v[:n] for k, v in ens['out'].items()}
    e['corners_out'] = e['corners_out'].reshape(n, 8, 3)
    prob = np.asarray([m[4] for m in meta], np.float32)

    # the conditions that keep the test from hiding a failure
    low_view, low_mask = ~(d.view_iou >= A), ~(d.mask_in_box >= M)
    assert 0 < low_view.sum() < n and 0 < low_mask.sum() < n, (low_view, low_mask)
    accept = ~low_view & ~low_mask
    assert np.array_equal(d.accept, accept) and np.array_equal(d.view_iou, d0.view_iou) and np.array_equal(d.mask_in_box, d0.mask_in_box)
    offsets, members = NMS.groups_of([m[1] for m in meta], [DT.type2class[m[2]] for m in meta])
    assert len(offsets) - 1 == n // 2 and (np.diff(offsets) == 2).all()                 # 9 groups of two
    partner = np.zeros(n, np.int64)                  # the other report of the same object
    partner[members[0::2]], partner[members[1::2]] = members[1::2], members[0::2]
    assert all(np.array_equal(np.asarray(meta[i][3]) + SHIFT, meta[partner[i]][3]) for i in range(n) if prob[i] > prob[partner[i]])
    freed = [i for i in range(n) if accept[i] and not accept[partner[i]] and prob[partner[i]] > prob[i]]
    assert freed and all(d.keep[i] and d.suppressed_by[i] == -1 for i in freed), (freed, accept, d.keep, d.suppressed_by)
    voted = np.nonzero(d.keep & (d.n_votes > 0))[0]
    assert len(voted) > 0

    # the ensemble: view 0 is the plain run, its output is the specification's on the run's own view labels
    assert ens['flip_mask'] == 0b10 and ens['metric'] == '3d' and ens['vote'] == 0.0
    held = EC.Held(ens, n)
    assert np.array_equal(held.labels.astype(np.float64), d.view_label) and d.view_label.shape == (2, n, 7)
    for i, r in enumerate(plain):
        assert np.array_equal(r['label'], d.view_label[0, i]) and r['score'] == d.view_score[0, i] == d.score[i], i
    unsure = [] if exact else [i for i, _ in held.bad('3d', 0.0)]
    assert len(unsure) <= n // 4, held.bad('3d', 0.0)
    want = held.expected('3d', 0.0)
    if exact:
        assert all(same(e[k], want[k]) for k in FE.OUTPUTS), [k for k in FE.OUTPUTS if not same(e[k], want[k])]
        worst = 0.0
    else:
        worst = EC.compare(held, e, want, 0.0, 'the ensemble of the stages', unsure)

    # NMS read the corners the ensemble wrote, ranked by prob, and listed exactly the accepted rows
    assert same(nms['corners'][:n], e['corners_out']) and same(nms['score'][:n], prob) and nms['threshold'] == NMS_IOU and nms['metric'] == '3d'
    assert sorted(nms['members'].tolist()) == np.nonzero(accept)[0].tolist()
    cache = {}
    spec_nms = FN.greedy_nms(nms['corners'], nms['score'], nms['offsets'], nms['members'], NMS_IOU, FN.IOU3D, cache=cache)
    assert all(abs(v[FN.IOU3D] - NMS_IOU) >= NC.MARGIN for v in cache.values()), cache
    NC.assert_equal((nms['keep'], nms['suppressed_by'], nms['rank']), spec_nms, 'the NMS of the stages')

    # the fusion read the ensemble's label and corners, and the weight is prob
    assert same(fuse['label'][:n], e['label_out']) and same(fuse['corners'][:n], e['corners_out']) and same(fuse['weight'][:n], prob)
    assert fuse['vote'] == NMS_IOU
    lo, ko, nv, clusters = FF.fuse_clusters(fuse['label'], fuse['corners'], fuse['weight'], nms['offsets'], nms['members'], *spec_nms, NMS_IOU,
                                            FN.IOU3D, cache=cache)
    assert np.array_equal(fuse['n_votes'], nv) and sorted(clusters) == voted.tolist()
    for i in range(n):
        if exact or i not in clusters:
            assert same(fuse['label_out'][i], lo[i]) and same(fuse['corners_out'][i], ko[i]), i
        else:
            b = FC.label_bounds(clusters[i], lo[i], NMS_IOU)
            err = np.abs(fuse['label_out'][i].astype(np.float64) - lo[i].astype(np.float64))
            kerr = np.abs(fuse['corners_out'][i].astype(np.float64) - ko[i].astype(np.float64)).max()
            kb = EC.corner_bound(b, lo[i], ko[i])
            assert (err <= b).all() and kerr <= kb, (i, err, b, kerr, kb)
            worst = max(worst, float((err / b).max()), kerr / kb)

    # the records: raw_* the ensemble's output; label / corners the fusion's for a kept box with voters, the ensemble's for every other
    f64 = lambda a: a.astype(np.float64)
    assert same(d.raw_label, f64(e['label_out'])) and same(d.raw_corners, f64(e['corners_out']))
    assert same(d.label, f64(fuse['label_out'][:n])) and same(d.corners, f64(fuse['corners_out'][:n]))
    rest = np.setdiff1d(np.arange(n), voted)
    assert same(d.label[rest], d.raw_label[rest]) and same(d.corners[rest], d.raw_corners[rest])
    assert all(not same(d.label[i], d.raw_label[i]) for i in voted)
    assert np.array_equal(d.n_votes, fuse['n_votes'][:n]) and np.array_equal(d.view_iou, f64(e['agreement']))
    assert np.array_equal(d.keep, nms['keep'][:n].astype(bool) & accept) and np.array_equal(d.suppressed_by, nms['suppressed_by'][:n])

    # the three log lines, in order, with the counts of the arrays
    fused = d.n_votes[d.n_votes > 0]
    assert lines == ['consistency: kept %d of %d (mask_in_box < %g: %d, view_iou < %g: %d)' % (accept.sum(), n, M, low_mask.sum(), A, low_view.sum()),
                     'tta: 2 views (1 mirrored), fused %d of %d boxes, mean view IoU %.4f' % ((d.n_views_voted > 0).sum(), n, d.view_iou.mean()),
                     'nms (3d IoU > %g, ranked by prob): kept %d of %d detections, fused %d boxes from %d votes'
                     % (NMS_IOU, d.keep.sum(), accept.sum(), len(fused), fused.sum())], lines
    if exact:
        assert (accept.sum(), low_mask.sum(), low_view.sum(), d.keep.sum(), len(fused), fused.sum()) == (11, 2, 6, 6, 5, 5), lines
        assert lines[1] == 'tta: 2 views (1 mirrored), fused 18 of 18 boxes, mean view IoU 0.5241', lines
        assert counter.n <= CPU_CALLS, counter.n

    # Detector.detect returns exactly the kept rows, and --vis_dir draws d.corners
    with Stages(rt) as vis:
        records = [r for recs in DT.Detector(flags(), rt=rt, **options).detect(scenes, dets, scene_ids=ids, vis_dir=str(root / 'pics')) for r in recs]
    kept = np.nonzero(d.keep)[0]
    assert len(records) == len(kept)
    for r, i in zip(records, kept):
        assert np.array_equal(r['box2d'], meta[i][3]) and r['prob'] == meta[i][4] and r['votes'] == d.n_votes[i] and r['view_iou'] == d.view_iou[i]
        assert same(r['label'], d.label[i]) and same(r['corners'], d.corners[i]) and r['mask_in_box'] == d.mask_in_box[i]
    assert vis.entry_points == cap.entry_points
    assert vis.render and all(same(k[:n], d.corners.astype(np.float32)) for k in vis.render)
    return ['%d detections in 2 views: %d accepted (%d below min_view_iou %.4f, %d below min_mask_in_box %.4f), %d kept, %d fused; '
            '%d freed by a rejected partner; worst share of a bound %.3f; %d near a tie; %d Tensor.cpu calls in decode_all'
            % (n, accept.sum(), low_view.sum(), A, low_mask.sum(), M, d.keep.sum(), len(fused), len(freed), worst, len(unsure), counter.n)]
