"""Shared cases of the t3d_detect_nms tests: the CPU tests run them through the NumPy specification library (fake_nms), the GPU tests
through libt3d.so, and both compare with fake_nms.greedy_nms.

The kernel decides in fp32, the specification in fp64, so no case may sit on a threshold: `Case.repair(metric, threshold)` computes every
same-group pair's IoU under that metric in fp64 on the fp32-rounded corners and redraws a box of any pair with |IoU - threshold| <
MARGIN until none is left -- the cases of every (metric, threshold) are repaired on their own IoUs, from the same seeds.  MARGIN = 1e-3
is 50 times the 2e-5 that tests/test_dataset_gpu.py holds the device IoU to against the same specification."""
import functools

import numpy as np
import torch

import fake_detect as FD
import fake_nms as FN
from transferable3d_amd import nms as NMS

MARGIN = 1e-3
THRESHOLDS = (0.25, 0.5)
METRICS = ('3d', 'bev')
METRIC_ID = {'3d': FN.IOU3D, 'bev': FN.IOU2D}
FILL = (7, -7, -9)            # what the outputs hold before a launch in these tests: an unlisted box must still hold it afterwards
MAX_REDRAWN = 0.05


_IOUS = {}


def memo_iou(k1, k2):
    """fake_nms.iou_corners, remembered by the boxes' bytes: the cases of the four (metric, threshold) pairs share most of their boxes."""
    key = (k1.tobytes(), k2.tobytes())
    if key not in _IOUS:
        _IOUS[key] = FN.iou_corners(k1, k2)
    return _IOUS[key]


def corners_of(box):
    """(cx, cy, cz, l, w, h, ry) -> [8, 3] fp32 in get_3d_box order (rows 0-3 the +h/2 face)."""
    cx, cy, cz, l, w, h, ry = box
    return FD.get_3d_box(l, w, h, ry, (cx, cy, cz)).astype(np.float32)


def draw_object(r):
    return np.concatenate([r.uniform([-3, -0.5, 1], [3, 0.5, 6]), r.uniform(0.4, 2.0, 3), [r.uniform(-np.pi, np.pi)]])


def draw_copy(r, obj):
    c = obj.copy()
    c[0:3] += r.normal(0, 0.12, 3)
    c[3:6] *= r.uniform(0.85, 1.15, 3)
    c[6] += r.normal(0, 0.15)
    return c


class Case:
    """Boxes, scores and groups of one call.  parent[i]: the object box i is a jittered copy of (None: a stray box), for redraws."""

    def __init__(self, name, seed=0):
        self.name, self.r = name, np.random.RandomState(seed)
        self.boxes, self.parent, self.scores, self.groups, self.unlisted = [], [], [], [], []
        self.cache, self.redrawn, self.hand_built = {}, 0, False

    def add_box(self, box, score, parent=None):
        self.boxes.append(np.asarray(box, np.float64))
        self.parent.append(parent)
        self.scores.append(score)
        return len(self.boxes) - 1

    def add_group(self, size, dup=4, clutter=0, spread=None):
        """A group of exactly `size` boxes: objects with 1..dup jittered copies each, then `clutter` stray boxes; random scores.
        spread: the objects' centres on a grid of that pitch instead of at random (well-separated objects: few pairs can touch)."""
        g, k = [], 0
        while len(g) < size - min(clutter, size):
            obj = draw_object(self.r)
            if spread:
                obj[0], obj[2], obj[3:6] = spread * (k % 16), spread * (k // 16), self.r.uniform(0.4, 1.0, 3)
            k += 1
            for _ in range(min(self.r.randint(1, dup + 1), size - min(clutter, size) - len(g))):
                g.append(self.add_box(draw_copy(self.r, obj), self.r.uniform(0, 1), obj))
        while len(g) < size:
            g.append(self.add_box(draw_object(self.r), self.r.uniform(0, 1)))
        self.groups.append(sorted(g))
        return g

    def add_unlisted(self, count):
        self.unlisted += [self.add_box(draw_object(self.r), self.r.uniform(0, 1)) for _ in range(count)]

    # ---- arrays ----
    @property
    def n(self):
        return len(self.boxes)

    def arrays(self):
        """(corners [n,8,3] fp32, score [n] fp32, group_offsets, members)"""
        corners = np.stack([corners_of(b) for b in self.boxes]) if self.boxes else np.zeros((0, 8, 3), np.float32)
        offsets = np.concatenate([[0], np.cumsum([len(g) for g in self.groups])]).astype(np.int32)
        members = np.asarray([b for g in self.groups for b in g], np.int32)
        return corners, np.asarray(self.scores, np.float32), offsets, members

    def repair(self, metric, threshold):
        """The margin rule (module docstring).  Asserts that at most MAX_REDRAWN of the boxes were redrawn."""
        self.metric, self.threshold = metric, threshold
        while True:
            corners, score, offsets, members = self.arrays()
            k64 = corners.astype(np.float64)
            bad = set()
            for g in self.groups:
                FN.group_pairs(k64, score, np.asarray(g, np.int64), self.cache, memo_iou)
            for (i, j), ious in self.cache.items():
                if abs(ious[METRIC_ID[metric]] - threshold) < MARGIN:
                    bad.add(j)
            if not bad:
                break
            for j in bad:
                self.boxes[j] = draw_copy(self.r, self.parent[j]) if self.parent[j] is not None else draw_object(self.r)
                self.cache = {k: v for k, v in self.cache.items() if j not in k}
            self.redrawn += len(bad)
        assert self.redrawn <= MAX_REDRAWN * self.n, '%s: %d of %d boxes redrawn' % (self.name, self.redrawn, self.n)
        return self

    def expected(self):
        """(keep, suppressed_by, rank) of the specification under the case's metric and threshold, unlisted boxes at FILL."""
        corners, score, offsets, members = self.arrays()
        return FN.greedy_nms(corners, score, offsets, members, self.threshold, METRIC_ID[self.metric], fill=FILL, cache=self.cache)


def hand_case(name, boxes, scores, groups, metric, threshold):
    c = Case(name)
    c.hand_built, c.metric, c.threshold = True, metric, threshold
    for b, s in zip(boxes, scores):
        c.add_box(b, s)
    c.groups = [sorted(g) for g in groups]
    return c


def unit_cube(dx, score=None, size=1.0):
    """An axis-aligned cube of edge `size` shifted by dx along x: two of them overlap in a slab of (size - |dx|) * size^2."""
    return (dx, 0.0, 3.0, size, size, size, 0.0)


COMBOS = [(m, t) for m in METRICS for t in THRESHOLDS]


@functools.lru_cache(maxsize=None)
def cases(metric='3d', threshold=0.5):
    """name -> Case (repaired for this metric and threshold; built once per process and shared by the tests: nothing changes them)."""
    out = {}
    hand = lambda name, boxes, scores, groups: hand_case(name, boxes, scores, groups, metric, threshold)
    for k, size in enumerate((1, 2, 63, 64, 65, 130)):       # both sides of a wave and of a 64-bit mask word, and more than two words
        c = Case('size_%d' % size, seed=(11, 12, 13, 14, 15, 16)[k])
        c.add_group(size, dup=2 if size == 2 else 4, clutter=size // 8)
        out[c.name] = c.repair(metric, threshold)
    c = Case('size_260', seed=21)                             # five words per row: the sweep's eight lanes per group
    c.add_group(260, dup=4, spread=3.0)
    out[c.name] = c.repair(metric, threshold)
    c = Case('mixed_40', seed=31)                             # 40 groups of 0..12 boxes, boxes listed in no group between them
    for g, size in enumerate(list(range(13)) * 3 + [0]):
        if size:
            c.add_group(size, dup=3, clutter=size // 5)
        else:
            c.groups.append([])
        if g % 7 == 3:
            c.add_unlisted(2)
    assert len(c.groups) == 40
    out[c.name] = c.repair(metric, threshold)
    # A (0) covers B (1) at IoU 3/5 (a shift of a quarter edge), B covers C (2) likewise, A and C overlap by half an edge: IoU 1/3
    out['chain'] = hand('chain', [unit_cube(0.0), unit_cube(0.25), unit_cube(0.5)], [0.9, 0.8, 0.7], [[0, 1, 2]])
    # equal scores: the lower index wins; a NaN ranks last, behind a real -inf of a lower index and before one of a higher index
    out['ties_nan'] = hand('ties_nan', [unit_cube(0.0), unit_cube(0.1), unit_cube(5.0), unit_cube(5.1), unit_cube(9.0), unit_cube(9.1),
                                             unit_cube(9.2)],
                                [0.5, 0.5, np.nan, 0.1, -np.inf, np.nan, -np.inf], [[0, 1, 2, 3, 4, 5, 6]])
    out['identical'] = hand('identical', [unit_cube(0.0), unit_cube(0.0), draw_object(np.random.RandomState(5))], [0.3, 0.6, 0.9],
                                 [[0, 1], [2]])
    flat = (0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.3)               # no length, width or height: IoU 0 / 0 under both metrics
    out['zero_volume'] = hand('zero_volume', [flat, flat, unit_cube(4.0), unit_cube(4.1)], [0.9, 0.8, 0.7, 0.6], [[0, 1, 2, 3]])
    return out


@functools.lru_cache(maxsize=None)
def big_case(metric='3d', threshold=0.25):
    """One group of exactly T3D_DETECT_NMS_MAX_GROUP boxes: 256 well-separated objects x 4 copies."""
    c = Case('group_1024', seed=41)
    k = 0
    g = []
    for k in range(256):
        obj = draw_object(c.r)
        obj[0], obj[2], obj[3:6] = 3.0 * (k % 16), 3.0 * (k // 16), c.r.uniform(0.4, 1.0, 3)
        g += [c.add_box(draw_copy(c.r, obj), c.r.uniform(0, 1), obj) for _ in range(4)]
    c.groups.append(sorted(g))
    return c.repair(metric, threshold)


@functools.lru_cache(maxsize=None)
def expected(name, metric, threshold):
    c = big_case(metric, threshold) if name == 'group_1024' else cases(metric, threshold)[name]
    want = c.expected()
    listed = [b for g in c.groups for b in g]
    if not c.hand_built and len(listed) > 1:       # a case that suppresses nothing, or everything it can, checks little
        assert want[0][listed].min() == 0 and want[0][listed].max() == 1, (name, metric, threshold)
    for a in want:
        a.setflags(write=False)
    return want


def run(rt, corners, score, offsets, members, threshold, metric):
    """nms.DeviceNms on NumPy arrays, outputs pre-filled with FILL -> (keep, suppressed_by, rank) as NumPy arrays."""
    dev = NMS.DeviceNms(rt)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)
    k = up(corners.reshape(-1, 24)) if len(corners) else rt.zeros(0, 24)
    s = up(score) if len(score) else rt.zeros(0)
    out = dev.run(k, s, offsets, members, threshold, metric, fill=FILL)
    return tuple(t.cpu().numpy().copy() for t in out)


def run_case(rt, c):
    return run(rt, *c.arrays(), c.threshold, c.metric)


def assert_equal(got, want, what):
    for k, g, w in zip(('keep', 'suppressed_by', 'rank'), got, want):
        assert np.array_equal(g, w), (what, k, np.nonzero(g != w)[0][:8], g[g != w][:8], w[g != w][:8])


def moved(rt, names, metric, threshold, seed=0):
    """The groups of the cases `names` in one larger call, at permuted box indices, in reversed group order and with unlisted boxes
    in between -> per case, the answers mapped back to the case's own indices (suppressed_by through the permutation)."""
    cs = [cases(metric, threshold)[k] for k in names]
    r = np.random.RandomState(seed)
    total = sum(c.n for c in cs) + 9
    perm = r.permutation(total)
    corners, score = np.zeros((total, 8, 3), np.float32), np.zeros(total, np.float32)
    groups, where, at = [], [], 0
    for c in cs:
        k, s, _, _ = c.arrays()
        new = np.sort(perm[at:at + c.n])          # interleaved with the other cases' boxes; ascending, so that equal scores tie as before
        at += c.n
        if c.n:
            corners[new], score[new] = k, s
        where.append(new)
        groups = [sorted(int(new[b]) for b in g) for g in c.groups] + groups
    for j in perm[at:]:
        corners[j] = corners_of(draw_object(r))
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    members = np.asarray([b for g in groups for b in g], np.int32)
    keep, sup, rank = run(rt, corners, score, offsets, members, threshold, metric)
    assert all(keep[j] == FILL[0] and sup[j] == FILL[1] and rank[j] == FILL[2] for j in perm[at:])
    back = np.full(total, -1, np.int64)
    out = []
    for c, new in zip(cs, where):
        back[:] = -1
        back[new] = np.arange(c.n)
        s = sup[new]
        listed = np.zeros(c.n, bool)
        listed[[b for g in c.groups for b in g]] = True
        out.append((keep[new], np.where(listed & (s >= 0), back[np.clip(s, 0, total - 1)], s).astype(np.int32), rank[new]))
    return out


# ---- scene-level flow ---------------------------------------------------------------------------------------------------------------
# detect_check.write_data_set's data set with every label detection written a second time, at a lower prob and with its 2-D box
# shifted by two pixels: the duplicate a 2-D detector hands over.  Same-group IoUs of the run without suppression, as measured on
# the specification libraries (3-D metric; rank order, better box first), are listed by `check_flow`'s report; FLOW_T is the first of
# (0.25, 0.2, 0.3, 0.15, 0.35) that keeps MARGIN from all of them and removes at least one line, and leaves at least one, per scene.
FLOW_CANDIDATES = (0.25, 0.2, 0.3, 0.15, 0.35)
FLOW_T = 0.25


def write_duplicated(root):
    """-> (ids, detection folder, index file, detections per scene)"""
    import os
    import detect_check as DC
    ids, _, idx, dets = DC.write_data_set(root)
    folder = os.path.join(str(root), 'det_duplicated')
    os.makedirs(folder)
    out = []
    for s, rows in zip(ids, dets):
        rows = list(rows) + [(name, tuple(v + 2.0 for v in b), p - 0.4) for name, b, p in rows if (name, b, p) != DC.SPARSE]
        out.append(rows)
        with open(os.path.join(folder, '%06d.txt' % s), 'w') as fh:
            for name, b, p in rows:
                fh.write('%s -1 -10 -10 %r %r %r %r -1 -1 -1 -1000 -1000 -1000 -10 %r\n' % ((name,) + b + (p,)))
    return ids, folder, idx, out


def records_nms(ids, records, threshold, metric='3d', score='prob'):
    """fake_nms.greedy_nms over the records of an unsuppressed Detector.detect -> (records without the suppressed ones, same-group IoUs
    under the metric, records per scene before, after)."""
    from transferable3d_amd.constants import type2class
    flat = [(s, r) for s, recs in zip(ids, records) for r in recs]
    corners = np.stack([r['corners'] for _, r in flat]).astype(np.float32)
    sc = np.asarray([r[score] for _, r in flat], np.float32)
    offsets, members = NMS.groups_of([s for s, _ in flat], [type2class[r['class']] for _, r in flat])
    cache = {}
    keep, _, _ = FN.greedy_nms(corners, sc, offsets, members, threshold, METRIC_ID[metric], cache=cache)
    kept, i = [], 0
    for recs in records:
        kept.append([r for k, r in enumerate(recs) if keep[i + k]])
        i += len(recs)
    return kept, sorted(v[METRIC_ID[metric]] for v in cache.values())


def check_flow(rt, root, threshold=FLOW_T):
    """detect --nms_iou against the specification applied to the unsuppressed run, the two-step route and Detector.detect; -> report lines."""
    import os
    import detect_check as DC
    from transferable3d_amd import detect as DT, semisup_infer as SI, sunrgbd_data as SD, test_semisup as TS
    from transferable3d_amd.dataset import save_zipped_pickle
    quiet = lambda *a: None
    ids, folder, idx, dets = write_duplicated(root)
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS
    res = lambda name: os.path.join(str(root), name)
    DT.main(base + ['--result_dir', res('plain')], rt=rt, log=quiet)
    plain = DC.read_results(res('plain'))
    scenes = DC.load_scenes(root, ids)
    records = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt).detect(scenes, dets, scene_ids=ids)
    assert all(r['corners'].shape == (8, 3) for recs in records for r in recs)
    lines = DC.record_lines(ids, records)
    assert all(lines.get(c, '') == t for c, t in plain.items()), 'without the flags: the files are the records, all of them'
    kept, ious = records_nms(ids, records, threshold)
    report = ['same-group 3-D IoUs of the unsuppressed run: ' + ' '.join('%.4f' % v for v in ious)]
    good = [t for t in FLOW_CANDIDATES
            if all(abs(v - t) >= MARGIN for v in ious)
            and all(0 < len(k) < len(r) for k, r in zip(records_nms(ids, records, t)[0], records))]
    assert good and good[0] == threshold, (good, ious)
    want = DC.record_lines(ids, kept)
    logged = []
    DT.main(base + ['--result_dir', res('nms'), '--nms_iou', str(threshold)], rt=rt, log=logged.append)
    got = DC.read_results(res('nms'))
    n_all, n_kept = sum(len(r) for r in records), sum(len(k) for k in kept)
    assert all(want.get(c, '') == t for c, t in got.items()) and set(want) <= set(got), 'detect --nms_iou differs from the specification on the unsuppressed run'
    assert any('kept %d of %d detections' % (n_kept, n_all) in l for l in logged), logged
    for c, t in got.items():                                         # exactly the lines of the plain run, minus the suppressed ones, in its order
        left = iter(plain[c].splitlines())
        assert all(any(l == m for m in left) for l in t.splitlines()), c
    # the two-step route with the same flags
    lists = SD.extract_roi_seg_from_rgb_detection(folder, str(root), valid_id_list=ids, seed=3, rt=rt)
    path = res('val_det_dup.zip.pickle')
    save_zipped_pickle(lists, path)
    two = lambda name, extra: SI.test(SI.build_flags(DC.MODEL_FLAGS + ['--from_rgb_detection', '--data_path', path, '--result_dir', res(name),
                                                                       '--device_decode'] + extra), rt=rt, log=quiet)
    p = two('two_step_nms', ['--nms_iou', str(threshold)])
    assert DC.read_results(res('two_step_nms')) == got, 'semisup_infer --device_decode --nms_iou differs from detect --nms_iou'
    assert len(p[3]) == len(p.decoded) == n_kept and p.decoded.keep.all()
    q = two('two_step_plain', [])
    assert DC.read_results(res('two_step_plain')) == plain and q.decoded.keep is None and q.decoded.suppressed_by is None
    # Detector.detect and Detector.predictions
    det = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, nms_iou=threshold)
    assert DC.record_lines(ids, det.detect(scenes, dets, scene_ids=ids)) == want
    report.append('threshold %.2f: %d of %d detections kept, %d classes' % (threshold, n_kept, n_all, len(got)))
    return report
