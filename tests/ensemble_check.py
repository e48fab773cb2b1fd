"""Shared cases and comparison of the t3d_detect_ensemble tests: the CPU tests run them through the NumPy specification library
(fake_ensemble), the GPU tests through libt3d.so, and both compare with fake_ensemble.ensemble.

Cases: a detection is an object box (nms_check.draw_object); its views are nms_check.draw_copy jitters of it (in seven detections of
ten one view is the object itself), a mirrored view is stored mirrored; some views are stray boxes 20 m away, some the same box written
with l and w exchanged and the heading turned by pi/2, some labels hold a NaN; the weights include 0, a negative value, NaN and inf.  Sizes
(n, V): (1, 1), (1, 8), (63, 2), (64, 3), (65, 8), (257, 5), (64, 1) -- both sides of a wave, more than a 256-thread block, every pair
count (0, 1, 3, 10, 28), so the pair threads of a wave straddle detections -- and four hand-built cases: one 45 m from the origin, one
with all views identical (exact ties: anchor 0, agreement 1), one whose view 0 is the outlier (the anchor is not 0), one of non-finite
labels and angles.  Passes: both metrics, a vote threshold of 0 and of 0.5.

The kernel computes the IoUs in fp32 and the specification in fp64, so four conditions hold on every generated case -- conditions on the
inputs, not measurements; a detection that breaks one is redrawn whole (`repair`), at most nms_check.MAX_REDRAWN of the detections of a
pass's generated cases taken together (`cases` asserts it; at eight views the second condition alone redraws about one detection in
twenty-five, the eight mean IoUs lying within some 0.1 of each other, so the cap is not put on that case alone):
  * no IoU of a valid view with the anchor within nms_check.MARGIN of the vote threshold (an IoU of exactly 0 -- a stray 20 m away,
    whose edges never meet the other box's, on the device as in the specification -- is not near a threshold of 0);
  * the best and the second-best anchor mean more than MARGIN apart, unless they are equal (an exact tie comes from the same IoUs
    summed in the same order: two valid views, or all but two of them strays);
  * no voter whose heading difference to the anchor, modulo pi/2, lies within fuse_check.ALIGN_MARGIN of pi/4;
  * no un-mirrored heading within MARGIN of +-pi, where `wrap` jumps.

Comparison (`compare`): anchor, n_votes and which rows are byte copies of view 0, exactly.  agreement and min_iou within
fuse_check.IOU_BOUND = 2e-5, the project's bound on the device IoU (the corners are built in fp32 on both sides; the device's sine and
cosine differ from the rounded fp64 ones by an ulp or two of a coordinate).  A fused label entry within
2 * (IOU_BOUND / max(vote threshold, smallest voting IoU)) * spread + 4 ulp, fuse_check's derivation with the voters' smallest IoU in the
place of V where the vote threshold is 0; the corners with that bound carried through the decode formula.  An anchor other than view 0
with nothing fused: its view label within 4 ulp (the fp64 sine and cosine of the mirror), the corners likewise."""
import functools

import numpy as np
import torch

import fake_ensemble as FE
import fuse_check as FC
import nms_check as NC
from transferable3d_amd import ensemble as EN

IOU_BOUND, ALIGN_MARGIN, MARGIN = FC.IOU_BOUND, FC.ALIGN_MARGIN, NC.MARGIN
FILL = (-7.5, -9.5, -3.5, -4.5, -5, -6)          # what the six outputs hold before a launch in these tests
PASSES = [(m, t) for m in NC.METRICS for t in (0.0, 0.5)]
SIZES = ((1, 1, 0), (1, 8, 0b10101010), (63, 2, 0b10), (64, 3, 0b010), (65, 8, 0b10101010), (257, 5, 0b01010), (64, 1, 0))
WEIGHTS = (0.0, -1.0, np.nan, np.inf)


def mirrored(label, angle):
    """What a mirrored view holds for the box `label`: the mirror is its own inverse."""
    return FE.unmirror(np.asarray(label, np.float32), angle)


def turned(box):
    """The same box written with l and w exchanged and the heading turned by pi/2."""
    cx, cy, cz, l, w, h, ry = box
    return np.asarray([cx, cy, cz, w, l, h, ry + np.pi / 2.0])


def stray(r):
    b = NC.draw_object(r)
    b[0] += 20.0 + r.uniform(0, 20.0)
    return b


class Case:
    """labels [V, n, 7] and weights [V, n] fp32, rot [n] fp32 (or None), flip_mask; `draw(i)` draws detection i again."""

    def __init__(self, name, n, V, flip_mask, seed=0, far=False, with_rot=True):
        self.name, self.n, self.V, self.flip_mask, self.far = name, n, V, flip_mask, far
        self.r = np.random.RandomState(seed)
        self.labels, self.weights = np.zeros((V, n, 7), np.float32), np.zeros((V, n), np.float32)
        self.rot = np.zeros(n, np.float32) if with_rot else None
        self.redrawn, self.hand_built = 0, False
        for i in range(n):
            self.draw(i)

    def draw(self, i):
        r = self.r
        obj = NC.draw_object(r)
        if self.far:
            obj[0], obj[2] = obj[0] + 40.0, obj[2] + 18.0
        if self.rot is not None:
            self.rot[i] = np.pi / 2 + r.uniform(-0.6, 0.6)
        strength = np.ones(self.V)
        if r.uniform() < 0.7:
            strength[r.randint(self.V)] = 0.0
        for v in range(self.V):
            k = r.uniform()
            box = obj + strength[v] * (NC.draw_copy(r, obj) - obj)
            if k < 0.08:
                box = stray(r)
            elif k < 0.18:
                box = turned(box)
            label = FC.label_of(box)
            if (self.flip_mask >> v) & 1:
                label = mirrored(label, 0.0 if self.rot is None else self.rot[i])
            if 0.18 <= k < 0.21:
                label[r.randint(7)] = np.nan
            self.labels[v, i] = label
            w = r.uniform()
            self.weights[v, i] = WEIGHTS[r.randint(4)] if w < 0.08 else w

    def corners0(self):
        return np.stack([FE.label_corners(l) for l in self.labels[0]]) if self.n else np.zeros((0, 8, 3), np.float32)

    def expected(self, metric, vote):
        return FE.ensemble(self.labels, self.weights, self.flip_mask, self.rot, self.corners0(), vote, NC.METRIC_ID[metric], iou=NC.memo_iou)

    def bad(self, metric, vote):
        """The detections that break a condition of the module docstring."""
        want = self.expected(metric, vote)
        out = []
        for i in range(self.n):
            a, I, means = int(want['anchor'][i]), want['ious'].get(i, {}), want['means'].get(i, {})
            why = None
            for (u, v), x in I.items():
                if a in (u, v) and abs(x - vote) < MARGIN and not (x == 0.0 and vote == 0.0):
                    why = 'an IoU with the anchor near the vote threshold'
            top = sorted(means.values(), reverse=True)
            if len(top) > 2 and 0.0 < top[0] - top[1] < MARGIN:
                why = 'two anchor means too close'
            L = want['views'][:, i].astype(np.float64)
            for v, _ in want['voters'].get(i, []):
                if abs((L[v, 6] - L[a, 6]) % (np.pi / 2.0) - np.pi / 4.0) < ALIGN_MARGIN:
                    why = 'a voter near a tie of the quarter turns'
            for v in range(self.V):
                if (self.flip_mask >> v) & 1 and np.isfinite(L[v, 6]) and abs(abs(L[v, 6]) - np.pi) < MARGIN:
                    why = 'an un-mirrored heading near +-pi'
            if why:
                out.append((i, why))
        return out

    def repair(self, metric, vote):
        while True:
            bad = self.bad(metric, vote)
            if not bad:
                break
            for i, _ in bad:
                self.draw(i)
            self.redrawn += len(bad)
        return self


def hand_case(name, boxes, weights, flip_mask=0, rot=None):
    """boxes [n][V] of (cx, cy, cz, l, w, h, ry) or label rows of 7 under the key 'label'; never redrawn."""
    n, V = len(boxes), len(boxes[0])
    c = Case(name, 0, V, flip_mask)
    c.n, c.hand_built = n, True
    c.rot = None if rot is None else np.asarray(rot, np.float32)
    c.labels, c.weights = np.zeros((V, n, 7), np.float32), np.asarray(weights, np.float32).reshape(n, V).T.copy()
    for i in range(n):
        for v in range(V):
            b = boxes[i][v]
            label = np.asarray(b['label'], np.float32) if isinstance(b, dict) else FC.label_of(b)
            if (flip_mask >> v) & 1 and not isinstance(b, dict):
                label = mirrored(label, 0.0 if rot is None else c.rot[i])
            c.labels[v, i] = label
    return c


def hand_cases():
    r = np.random.RandomState(77)
    out = {}
    obj = NC.draw_object(r)
    out['identical'] = hand_case('identical', [[obj] * 5, [NC.unit_cube(0.0)] * 5], [[0.5] * 5, [0.2, 0.9, 0.1, 0.3, 0.4]])
    # view 0 is a poor copy (half a box off), the others sit on the object: the medoid is one of them
    off = obj.copy()
    off[0] += 0.5 * obj[3]
    tight = lambda: obj + np.concatenate([r.normal(0, 0.01, 3), np.zeros(4)])
    out['outlier0'] = hand_case('outlier0', [[off, tight(), tight(), tight()], [stray(r), tight(), tight(), tight()]],
                                [[0.9, 0.5, 0.5, 0.5]] * 2, flip_mask=0b0100, rot=[1.9, 1.2])
    nan = {'label': [np.nan] * 7}
    inf = {'label': list(FC.label_of(obj)[:6]) + [np.inf]}
    out['non_finite'] = hand_case('non_finite', [[nan, nan, nan], [nan, obj, inf], [obj, nan, obj + 0.01], [obj, obj + 0.01, obj + 0.02]],
                                  [[0.5] * 3] * 4, flip_mask=0b100, rot=[1.5, 1.5, 1.5, np.nan])
    return out


@functools.lru_cache(maxsize=None)
def cases(metric, vote):
    """name -> Case, built from the same seeds for every pass and repaired for this one; shared by the tests, which change nothing."""
    out = {}
    for k, (n, V, mask) in enumerate(SIZES):
        out['n%d_v%d' % (n, V)] = Case('n%d_v%d' % (n, V), n, V, mask, seed=101 + k, with_rot=k != 2).repair(metric, vote)
    out['far_45m'] = Case('far_45m', 40, 4, 0b1010, seed=131, far=True).repair(metric, vote)
    redrawn, total = sum(c.redrawn for c in out.values()), sum(c.n for c in out.values())
    assert redrawn <= NC.MAX_REDRAWN * total, '%s, vote threshold %g: %d of %d detections redrawn' % (metric, vote, redrawn, total)
    for name, c in hand_cases().items():
        if not c.bad(metric, vote):                      # (a hand-built case is never redrawn: a pass it does not suit leaves it out)
            out[name] = c
    return out


@functools.lru_cache(maxsize=None)
def expected_of(name, metric, vote):
    return cases(metric, vote)[name].expected(metric, vote)


# ---- running ------------------------------------------------------------------------------------------------------------------------
def run(rt, labels, weights, corners0, flip_mask, rot, vote, metric, fill=FILL):
    """ensemble.DeviceEnsemble on NumPy arrays, every output pre-filled -> the six outputs as NumPy arrays (corners [n, 8, 3]); the
    inputs must come back as they went."""
    V, n = labels.shape[:2]
    up = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device) if a.size else rt.zeros(0, *shape)
    d_labels, d_weights = [up(labels[v], 7) for v in range(V)], [up(weights[v]) for v in range(V)]
    d_corners, d_rot = up(corners0.reshape(-1, 24), 24), (None if rot is None else up(rot))
    dev = EN.DeviceEnsemble(rt)
    out = dev.run(d_labels, d_weights, d_corners, flip_mask, d_rot, vote, metric, fill=fill)
    back = lambda t: t.cpu().numpy().copy()
    for t, a in list(zip(d_labels, labels)) + list(zip(d_weights, weights)) + [(d_corners, corners0)] + ([] if rot is None else [(d_rot, rot)]):
        assert back(t).tobytes() == np.ascontiguousarray(a).tobytes(), 'an input was written'
    got = [back(t) for t in out]
    got[1] = got[1].reshape(-1, 8, 3)
    return dict(zip(FE.OUTPUTS, got))


def run_case(rt, c, metric, vote):
    return run(rt, c.labels, c.weights, c.corners0(), c.flip_mask, c.rot, vote, metric)


# ---- comparing ----------------------------------------------------------------------------------------------------------------------
ulp = FC.ulp


def corner_bound(b, want_label, want_corners):
    h, w, l = (float(v) for v in want_label[:3])
    half = 0.5 * np.sqrt(h * h + w * w + l * l)
    return b[3] + b[4] + b[5] + 0.5 * (b[0] + b[1] + b[2]) + half * b[6] + 8.0 * ulp(np.abs(want_corners).max() + half)


def compare(c, got, want, vote, what, unsure=()):
    """-> the worst share of a bound that was used (for the report).  unsure: detections whose inputs break a condition of the module
    docstring (the flow's, which nobody draws): their agreement and min_iou are compared, their decisions and boxes are not."""
    sure = np.setdiff1d(np.arange(c.n), list(unsure))
    for k in ('anchor', 'n_votes'):
        assert np.array_equal(got[k][sure], want[k][sure]), (what, k, np.nonzero(got[k] != want[k])[0][:8])
    corners0 = c.corners0()
    worst = 0.0
    for k in ('agreement', 'min_iou'):
        err = np.abs(got[k].astype(np.float64) - want[k].astype(np.float64))
        assert (err <= IOU_BOUND).all(), (what, k, int(err.argmax()), float(err.max()))
        worst = max(worst, float(err.max()) / IOU_BOUND if len(err) else 0.0)
    for i in sure:
        a = int(want['anchor'][i])
        if i not in want['fused'] and a <= 0:
            assert got['label_out'][i].tobytes() == c.labels[0, i].tobytes() and got['corners_out'][i].tobytes() == corners0[i].tobytes(), \
                (what, 'not a byte copy', i)
            continue
        wl = want['label_out'][i]
        b = np.asarray([4.0 * ulp(v) for v in wl])
        if i in want['fused']:
            low = min(x for _, x in want['voters'][i])
            b = FC.label_bounds(want['fused'][i], wl, max(vote, low))
        err = np.abs(got['label_out'][i].astype(np.float64) - wl.astype(np.float64))
        assert (err <= b).all(), (what, 'label', i, err, b)
        kb = corner_bound(b, wl, want['corners_out'][i])
        kerr = np.abs(got['corners_out'][i].astype(np.float64) - want['corners_out'][i].astype(np.float64)).max()
        assert kerr <= kb, (what, 'corners', i, kerr, kb)
        worst = max(worst, float((err / b).max()), kerr / kb)
    return worst


def check_case(rt, name, metric, vote):
    """One case on `rt` against the specification -> a report line."""
    c, want = cases(metric, vote)[name], expected_of(name, metric, vote)
    worst = compare(c, run_case(rt, c, metric, vote), want, vote, name)
    return '%-10s %3d x %d views: %3d fused from %3d votes, %3d anchored off view 0, worst share of a bound %.3f' % (
        name, c.n, c.V, len(want['fused']), int(want['n_votes'].sum()), int((want['anchor'] > 0).sum()), worst)


def moved(rt, name, metric, vote, pad=70, seed=0):
    """The detections of a case at permuted row indices of a larger call, other detections between them -> the six outputs at the case's
    own rows."""
    c = cases(metric, vote)[name]
    r = np.random.RandomState(seed)
    other = Case('pad', pad, c.V, c.flip_mask, seed=seed + 1, with_rot=c.rot is not None)
    total = c.n + pad
    perm = r.permutation(total)
    rows, rest = perm[:c.n], perm[c.n:]
    labels, weights = np.zeros((c.V, total, 7), np.float32), np.zeros((c.V, total), np.float32)
    labels[:, rows], labels[:, rest], weights[:, rows], weights[:, rest] = c.labels, other.labels, c.weights, other.weights
    rot = None
    if c.rot is not None:
        rot = np.zeros(total, np.float32)
        rot[rows], rot[rest] = c.rot, other.rot
    corners0 = np.zeros((total, 8, 3), np.float32)
    corners0[rows], corners0[rest] = c.corners0(), other.corners0()
    got = run(rt, labels, weights, corners0, c.flip_mask, rot, vote, metric)
    return {k: v[rows] for k, v in got.items()}


# ---- scene-level flow ---------------------------------------------------------------------------------------------------------------
class Capture:
    """Records what the t3d_detect_ensemble call of a run read on the device: the weights, the angles, view 0's corners, the arguments."""

    def __enter__(self):
        self.calls, self.real = [], EN.DeviceEnsemble.run
        cap = self

        def run(dev, labels, weights, corners0, flip_mask=0, rot_angle=None, vote_threshold=0.0, metric='3d', fill=None):
            host = lambda t: t.detach().cpu().numpy().copy()
            cap.calls.append(dict(labels=np.stack([host(t).reshape(-1, 7) for t in labels]), weights=np.stack([host(t).reshape(-1) for t in weights]),
                                  corners0=host(corners0).reshape(-1, 8, 3), flip_mask=flip_mask, rot=None if rot_angle is None else host(rot_angle),
                                  vote=vote_threshold, metric=metric))
            return cap.real(dev, labels, weights, corners0, flip_mask, rot_angle, vote_threshold, metric, fill)

        EN.DeviceEnsemble.run = run
        return self

    def __exit__(self, *exc):
        EN.DeviceEnsemble.run = self.real


class Held:
    """The arrays of a captured call in the shape `compare` and `Case.bad` read a case in."""
    bad = Case.bad

    def __init__(self, call, n):
        self.n, self.V, self.flip_mask = n, len(call['labels']), call['flip_mask']
        self.labels, self.weights, self.rot, self._corners0 = call['labels'][:, :n], call['weights'][:, :n], call['rot'][:n], call['corners0'][:n]

    def corners0(self):
        return self._corners0

    def expected(self, metric, vote):
        return FE.ensemble(self.labels, self.weights, self.flip_mask, self.rot, self._corners0, vote, NC.METRIC_ID[metric], iou=NC.memo_iou)


def check_flow(rt, root, exact):
    """detect --tta 3 --tta_flip on the golden scenes against the specification applied to the run's own view labels, and --tta 2 against
    the plain run.  exact: `rt` runs the specification itself and everything is compared as bytes; otherwise within `compare`'s bounds.
    -> (report lines, the Decoded of the run, the scenes' pieces for further checks)."""
    import detect_check as DC
    from transferable3d_amd import detect as DT, test_semisup as TS
    ids, folder, idx, dets = DC.write_data_set(root)
    scenes = DC.load_scenes(root, ids)
    flags = lambda: TS.build_flags(DC.MODEL_FLAGS)
    plain = [r for recs in DT.Detector(flags(), rt=rt).detect(scenes, dets, scene_ids=ids) for r in recs]
    assert all('view_iou' not in r for r in plain)
    lines = []
    det = DT.Detector(flags(), rt=rt, tta=3, tta_flip=True, log=lines.append)
    with Capture() as cap:
        meta, d = det.decode_all([det.extract(scenes, dets, ids)])
    n = len(plain)
    assert len(cap.calls) == 1 and len(d) == n > 4 and d.view_label.shape == (3, n, 7) and d.view_score.shape == (3, n)
    call = cap.calls[0]
    assert call['flip_mask'] == 0b010 and call['metric'] == '3d' and call['vote'] == 0.0 and call['rot'] is not None
    held = Held(call, n)
    assert np.array_equal(held.labels.astype(np.float64), d.view_label)
    assert np.allclose(held.weights, np.exp(d.view_score), rtol=1e-6, atol=0)           # exp of the fp32 score, as the runtime's exp rounds it
    for i, r in enumerate(plain):                                    # view 0 is the plain run
        assert np.array_equal(r['label'], d.view_label[0, i]) and r['score'] == d.view_score[0, i] == d.score[i], i
    assert any(not np.array_equal(d.view_label[0, i], d.view_label[2, i]) for i in range(n)), 'view 2 drew the points of view 0'
    # (nobody draws these detections: one whose views break a condition of the module docstring is left to the exact comparison of the
    # CPU test, and here only its agreement and min_iou are compared)
    unsure = [] if exact else [i for i, _ in held.bad('3d', 0.0)]
    assert len(unsure) <= n // 4, held.bad('3d', 0.0)
    want = held.expected('3d', 0.0)
    got = dict(label_out=d.label.astype(np.float32), corners_out=d.corners.astype(np.float32), agreement=d.view_iou.astype(np.float32),
               min_iou=d.view_min_iou.astype(np.float32), anchor=d.anchor_view.astype(np.int32), n_votes=d.n_views_voted.astype(np.int32))
    if exact:
        assert all(got[k].tobytes() == want[k].tobytes() for k in FE.OUTPUTS), [k for k in FE.OUTPUTS if got[k].tobytes() != want[k].tobytes()]
        worst = 0.0
    else:
        worst = compare(held, got, want, 0.0, 'detect --tta 3 --tta_flip', unsure)
    assert len(want['fused']) > 0 and (d.view_iou > 0).any()
    assert lines == ['tta: 3 views (1 mirrored), fused %d of %d boxes, mean view IoU %.4f' % (len(want['fused']), n, float(d.view_iou.mean()))], lines
    # --tta 2 without --tta_flip: view 0 stays the plain run, nothing is mirrored
    det2 = DT.Detector(flags(), rt=rt, tta=2)
    with Capture() as cap2:
        _, d2 = det2.decode_all([det2.extract(scenes, dets, ids)])
    assert cap2.calls[0]['flip_mask'] == 0 and d2.view_label.shape == (2, n, 7)
    assert all(np.asarray(r['label'], np.float32).tobytes() == d2.view_label[0, i].astype(np.float32).tobytes() for i, r in enumerate(plain))
    assert (d2.anchor_view == 0).all()                               # two views tie: view 0
    report = ['%d detections in 3 views: %d fused from %d votes, %d anchored off view 0, view IoU %.3f .. %.3f, worst share of a bound %.3f; %d near a tie'
              % (n, len(want['fused']), int(want['n_votes'].sum()), int((want['anchor'] > 0).sum()), d.view_iou.min(), d.view_iou.max(), worst, len(unsure))]
    return report, d, dict(ids=ids, folder=folder, idx=idx, dets=dets, scenes=scenes, plain=plain, want=want, meta=meta)
