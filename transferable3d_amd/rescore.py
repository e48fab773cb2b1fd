"""One confidence from the label-free measures of a detection (t3d_rescore_features / _fit / _apply, csrc/rescore.hip).

`detect` ranks a 3-D box by the confidence of the 2-D detector that proposed it.  What the stages behind the decode measure -- the
decoded network score, how the box reprojects onto its 2-D box, how it sits on the segmented points, how far its augmented views agree
-- says whether the 3-D box is any good, and until now reached the result only as hard thresholds.  A `Model` is an L2-regularised
logistic regression from those measures to "the box is right", fitted on the device on the detections of the classes that carry 3-D
labels (the targets are what t3d_sunrgbd_eval says about them) and applied to every class:

    FEATURES        the named features, in the order of the bits of t3d.h's feature_mask
    Model           names, coefficients (raw feature units, the intercept last), mean, scale and how it was fitted; JSON save / load
    DeviceRescore   the buffers of the three calls for n detections and their launches; nothing is fetched in between
    RescoreRequest  what `semisup_infer.DeviceStages` needs to run the stage: the model, the 2-D confidences, min_rescore
"""
import ctypes as C
import json

import numpy as np
import torch

from . import abi
from .abi import dptr, fptr, iptr
from .consistency import Test, lies_below

TEST = Test('min_rescore', ('rescore_prob',), 'rescore_prob < %g', lies_below, ())       # the stage's rejecting test (consistency.Test)
FEATURES = abi.RESCORE_FEATURES
DEFAULT_FEATURES = FEATURES[:6]                    # view_iou exists only under --tta
TARGETS = ('overlap', 'tp')


def feature_mask(names):
    """The bit field of t3d_rescore_features for a list of feature names; ValueError for an unknown or repeated name, or none."""
    names = list(names)
    bad = [k for k in names if k not in FEATURES]
    if bad or not names or len(set(names)) != len(names):
        raise ValueError('rescore features must be distinct names out of %s, got %r' % (', '.join(FEATURES), names))
    return sum(1 << FEATURES.index(k) for k in names)


def ordered(names):
    """The names in the order of the columns of X (table order, whatever order they were given in)."""
    feature_mask(names)
    return [k for k in FEATURES if k in names]


def status_names(status):
    return [name for bit, name in sorted(abi.RESCORE_STATUS.items()) if status & bit]


def check_min_rescore(p):
    if p is None:
        return None
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError('--min_rescore must lie in [0, 1], got %r' % (p,))
    return p


def add_arguments(parser):
    parser.add_argument('--rescore', default=None, metavar='MODEL.json',
                        help='rescore every detection by this model (rescore.py): the suppression, the result files and the evaluation rank by rescore_prob; implies --consistency')
    parser.add_argument('--min_rescore', type=float, default=None, help='reject a detection whose rescored confidence lies below this (0..1); needs --rescore')


class Model:
    """A fitted rescoring model.  features: the names, in column order; coef [F+1]: raw feature units, the intercept last (what
    t3d_rescore_apply reads); coef_std, mean, scale: the same model on the standardised columns.  The rest says how it was fitted:
    target ('overlap' / 'tp'), overlap threshold, lam, the fitted classes, n_rows and n_pos, the final loss, the status bits by name,
    n_iter, and the held-out report (None for a fit on everything).  Python's float repr round-trips, so a model saved and loaded
    gives the bytes it gave before."""
    KEYS = ('features', 'coef', 'coef_std', 'mean', 'scale', 'target', 'threshold', 'lam', 'classes', 'n_rows', 'n_pos', 'loss', 'status', 'n_iter',
            'holdout')

    def __init__(self, features, coef, coef_std=None, mean=None, scale=None, target='overlap', threshold=0.25, lam=1e-3, classes=(), n_rows=0,
                 n_pos=0, loss=None, status=(), n_iter=0, holdout=None):
        self.features = ordered(features)
        F = len(self.features)
        vec = lambda v, n, fill: [float(x) for x in (np.full(n, fill) if v is None else np.asarray(v, np.float64).reshape(-1))]
        self.coef, self.coef_std = vec(coef, F + 1, 0.0), vec(coef_std, F + 1, 0.0)
        self.mean, self.scale = vec(mean, F, 0.0), vec(scale, F, 1.0)
        if len(self.coef) != F + 1 or len(self.coef_std) != F + 1 or len(self.mean) != F or len(self.scale) != F:
            raise ValueError('a model of %d features has %d coefficients and an intercept' % (F, F))
        if target not in TARGETS:
            raise ValueError('rescore target must be one of %s, got %r' % (', '.join(TARGETS), target))
        self.target, self.threshold, self.lam = target, float(threshold), float(lam)
        self.classes, self.n_rows, self.n_pos = [str(c) for c in classes], int(n_rows), int(n_pos)
        self.loss, self.status, self.n_iter, self.holdout = (None if loss is None else float(loss)), [str(s) for s in status], int(n_iter), holdout

    @property
    def mask(self):
        return feature_mask(self.features)

    def to_dict(self):
        return {k: getattr(self, k) for k in self.KEYS}

    def save(self, path):
        with open(path, 'w') as fh:
            json.dump(self.to_dict(), fh, indent=1)
            fh.write('\n')

    @classmethod
    def load(cls, path):
        with open(path) as fh:
            d = json.load(fh)
        missing = [k for k in ('features', 'coef') if k not in d]
        if missing:
            raise ValueError('%s is no rescoring model: no %s' % (path, ', '.join(missing)))
        return cls(**{k: d[k] for k in cls.KEYS if k in d})

    @classmethod
    def of(cls, model):
        """A Model as it is, a path loaded."""
        return model if isinstance(model, cls) else cls.load(model)


class RescoreRequest:
    """What `semisup_infer.inference(decode='device', rescore=...)` needs: the model, the 2-D detector's confidence of every detection
    (the first feature, and `prob` of the records), and min_rescore (or None): a detection whose rescored confidence lies below it is
    rejected by the one accept rule."""

    def __init__(self, model, prob, min_rescore=None):
        self.model = Model.of(model)
        self.prob = np.ascontiguousarray(prob, np.float32).reshape(-1)
        self.min_rescore = check_min_rescore(min_rescore)

    def __len__(self):
        return len(self.prob)


class DeviceRescore:
    """The buffers of the three calls for `n` detections and the features `names`, and their launches on the runtime's stream.
    X [n, F]; out [n] fp64 and out32 [n] fp32 (what the suppression stages rank by); the fit's outputs and workspace are allocated by
    the first `fit`."""

    def __init__(self, rt, n, names):
        self.rt, self.n, self.names = rt, int(n), ordered(names)
        self.mask, self.F = feature_mask(self.names), len(self.names)
        self.ld = self.F
        self.X = rt.zeros(max(self.n, 1), self.ld, dtype=torch.float64)
        self.out = rt.zeros(max(self.n, 1), dtype=torch.float64)
        self.out32 = rt.zeros(max(self.n, 1))
        self.coef = rt.zeros(self.F + 1, dtype=torch.float64)
        self.fit_out = self.workspace = None
        self.max_iter = 0

    def features(self, prob=None, score=None, reproj=None, counts=None, view_iou=None):
        """X from the stage buffers: prob [n] fp32, score [n] fp32, reproj [n,5] fp64 and counts [n,4] int32 of DeviceConsistency,
        view_iou [n] fp32 (the ensemble's agreement).  Only what the selected features read is needed."""
        for t, dt in ((prob, torch.float32), (score, torch.float32), (reproj, torch.float64), (counts, torch.int32), (view_iou, torch.float32)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and t.shape[0] >= self.n), 'a stage buffer of another type or length'
        if 'view_iou' in self.names and view_iou is None:
            raise ValueError('the feature view_iou is the agreement of the augmented views: it needs --tta')
        a = abi.RescoreFeaturesArgs(self.n, self.ld, self.mask, fptr(prob), fptr(score), dptr(reproj), iptr(counts), fptr(view_iou), dptr(self.X))
        abi.check(self.rt.lib.t3d_rescore_features(C.byref(a), self.rt.stream()), 't3d_rescore_features')

    def fit(self, y, r, lam, max_iter=30, gtol=0.0, X=None, n=None, ld=None):
        """Enqueue the fit of y [n] uint8 on the rows of X (default: the features' matrix) with the weights r [n] fp64; the outputs stay
        on the device (`coef` is what `apply` reads) until `fetch_fit`."""
        rt = self.rt
        X, n, ld = (self.X if X is None else X), (self.n if n is None else int(n)), (self.ld if ld is None else int(ld))
        assert y.dtype == torch.uint8 and r.dtype == torch.float64 and X.dtype == torch.float64
        max_iter = int(max_iter) or 30
        need = abi.rescore_fit_workspace_bytes(n)
        if self.workspace is None or self.workspace.numel() * 8 < need:
            self.workspace = rt.zeros(need // 8, dtype=torch.float64)
        if self.fit_out is None or self.max_iter != max_iter:
            F = self.F
            self.fit_out = dict(coef_std=rt.zeros(F + 1, dtype=torch.float64), mean=rt.zeros(F, dtype=torch.float64),
                                scale=rt.zeros(F, dtype=torch.float64), loss=rt.zeros(max_iter, dtype=torch.float64),
                                ints=rt.zeros(2, dtype=torch.int32), counts=rt.zeros(2, dtype=torch.int64))
            self.max_iter = max_iter
        o = self.fit_out
        a = abi.RescoreFitArgs(n, self.F, ld, max_iter, 0, dptr(X), abi.u8ptr(y), dptr(r), float(lam), float(gtol),
                               C.c_void_p(self.workspace.data_ptr()), self.workspace.numel() * 8, dptr(self.coef), dptr(o['coef_std']),
                               dptr(o['mean']), dptr(o['scale']), dptr(o['loss']), iptr(o['ints']),
                               C.cast(C.c_void_p(o['ints'][1:].data_ptr()), C.POINTER(C.c_uint32)),
                               C.cast(C.c_void_p(o['counts'].data_ptr()), abi.L), C.cast(C.c_void_p(o['counts'][1:].data_ptr()), abi.L))
        abi.check(rt.lib.t3d_rescore_fit(C.byref(a), rt.stream()), 't3d_rescore_fit')

    def fetch_fit(self):
        """-> dict of host values: coef, coef_std [F+1], mean, scale [F], loss [max_iter], n_iter, status, n_rows, n_pos."""
        o = self.fit_out
        host = lambda t: t.cpu().numpy().copy()
        ints, counts = host(o['ints']), host(o['counts'])
        return dict(coef=host(self.coef), coef_std=host(o['coef_std']), mean=host(o['mean']), scale=host(o['scale']), loss=host(o['loss']),
                    n_iter=int(ints[0]), status=int(ints[1]) & 0xffffffff, n_rows=int(counts[0]), n_pos=int(counts[1]))

    def load(self, model):
        """A model's coefficients on the device, for `apply`."""
        if ordered(model.features) != self.names:
            raise ValueError('the model reads %s, the buffers hold %s' % (', '.join(model.features), ', '.join(self.names)))
        self.coef.copy_(torch.from_numpy(np.asarray(model.coef, np.float64)))

    def apply(self, n_valid=None, X=None, n=None, ld=None):
        """out[:n_valid] and out32[:n_valid] from the coefficients on the device; the rows behind keep what they held."""
        X, n, ld = (self.X if X is None else X), (self.n if n is None else int(n)), (self.ld if ld is None else int(ld))
        assert n <= self.out.shape[0]
        a = abi.RescoreApplyArgs(n, n if n_valid is None else int(n_valid), self.F, ld, 0, dptr(X), dptr(self.coef), dptr(self.out), fptr(self.out32))
        abi.check(self.rt.lib.t3d_rescore_apply(C.byref(a), self.rt.stream()), 't3d_rescore_apply')


FIT_FLAGS = ('rescore_classes', 'rescore_target', 'rescore_lambda', 'rescore_holdout', 'rescore_features')


def add_fit_arguments(parser):
    parser.add_argument('--rescore_fit', default=None, metavar='MODEL.json',
                        help='fit a rescoring model on the detections of the classes with 3-D labels and write it here (needs --dataset_dir and --idx_path)')
    parser.add_argument('--rescore_classes', nargs='+', default=None, help='classes to fit on (default: the evaluated classes that have ground truth)')
    parser.add_argument('--rescore_target', choices=TARGETS, default=None,
                        help="what a positive is: 'overlap' (default): the best overlap with a box of its class reaches the evaluation's 0.25; 'tp': the evaluation's true positive")
    parser.add_argument('--rescore_lambda', type=float, default=None, help='the ridge on the standardised coefficients (default 1e-3)')
    parser.add_argument('--rescore_holdout', type=float, default=None,
                        help='share of the images, in [0, 1), held out of the fit for the report (default 0.5; 0: fit on everything)')
    parser.add_argument('--rescore_features', nargs='+', default=None, help='features of the model (default: %s)' % ' '.join(DEFAULT_FEATURES))


def fit_options(args):
    """The keyword arguments of `fit_parts` from parsed flags (None without --rescore_fit); ValueError where they contradict."""
    given = [f for f in FIT_FLAGS if getattr(args, f) is not None]
    if args.rescore_fit is None:
        if given:
            raise ValueError('%s describe the fit of --rescore_fit: they need it' % ' / '.join('--' + f for f in given))
        return None
    if args.rescore is not None or args.min_rescore is not None:
        raise ValueError('--rescore_fit fits a model, --rescore applies one: they do not go together')
    holdout = 0.5 if args.rescore_holdout is None else float(args.rescore_holdout)
    if not 0.0 <= holdout < 1.0:
        raise ValueError('--rescore_holdout must lie in [0, 1), got %r' % (holdout,))
    lam = 1e-3 if args.rescore_lambda is None else float(args.rescore_lambda)
    if not lam > 0.0:
        raise ValueError('--rescore_lambda must be above 0, got %r' % (lam,))
    names = ordered(args.rescore_features) if args.rescore_features is not None else None
    return dict(path=args.rescore_fit, classes=args.rescore_classes, target=args.rescore_target or 'overlap', lam=lam, holdout=holdout, features=names)


def log_loss(p, y):
    """The mean of -log of the probability given to what happened, p clamped to [1e-6, 1 - 1e-6] (as the logit_prob feature clamps)."""
    p = np.clip(np.asarray(p, np.float64), 1e-6, 1.0 - 1e-6)
    y = np.asarray(y, bool)
    return float(-np.mean(np.where(y, np.log(p), np.log(1.0 - p)))) if len(p) else None


def reliability(p, y, bins=10):
    """Ten equal bins of the predicted confidence: [{'lo', 'hi', 'n', 'mean_predicted', 'observed'}]."""
    p, y = np.asarray(p, np.float64), np.asarray(y, bool)
    k = np.minimum((p * bins).astype(np.int64), bins - 1)
    return [{'lo': b / bins, 'hi': (b + 1) / bins, 'n': int((k == b).sum()),
             'mean_predicted': float(p[k == b].mean()) if (k == b).any() else None,
             'observed': float(y[k == b].mean()) if (k == b).any() else None} for b in range(bins)]


def fit(detector, scenes, detections, dataset_dir, idx_list, scene_ids=None, batch_scenes=16, **options):
    """`fit_parts` on scenes and their 2-D detections, as `Detector.detect` takes them."""
    if len(scenes) != len(detections):
        raise ValueError('%d scenes, detections of %d' % (len(scenes), len(detections)))
    scene_ids = list(range(len(scenes))) if scene_ids is None else list(scene_ids)
    parts = [detector.extract(scenes[lo:lo + batch_scenes], detections[lo:lo + batch_scenes], scene_ids[lo:lo + batch_scenes])
             for lo in range(0, len(scenes), batch_scenes)]
    return fit_parts(detector, parts, dataset_dir, idx_list, **options)


def fit_parts(detector, parts, dataset_dir, idx_list, test_on='AB', classes=None, target='overlap', threshold=0.25, lam=1e-3, holdout=0.5,
              features=None, seed=0, path=None, log=print, max_iter=30):
    """Fit a Model on the detections of extracted parts (what detect's `main` holds) -> Model (saved to `path` where given).
    The scenes go through the pipeline once, as a sweep's do: the detector must have been built with consistency=True and without
    suppression, thresholds or a model.  Every class of `classes` (default: the classes of the set `test_on` that have ground truth among
    the images idx_list and a detection) is evaluated by t3d_sunrgbd_eval; a detection of them is a positive where its best overlap with a
    box of its class reaches `threshold` ('overlap': "the box is on an object"; duplicates are not penalised, no feature can see them) or
    where the evaluation calls it a true positive ('tp').  The images are split by a RandomState(seed) permutation: the share `holdout`
    is kept out of the fit (row weight 0), the model is fitted on the rest on the device (the features never leave it), and the held-out
    images give the report: per class and mean the AP by `prob` against the AP by `rescore_prob` (both through the device evaluation),
    the log-loss of both, and a ten-bin reliability table.  holdout = 0 fits on everything and reports nothing."""
    from . import evaluate_sunrgbd as ES
    if target not in TARGETS:
        raise ValueError('rescore target must be one of %s, got %r' % (', '.join(TARGETS), target))
    if not detector.consistency or detector.nms_iou is not None or detector.soft_nms is not None or any(t is not None for t in detector.thresholds) \
            or detector.min_view_iou is not None or detector.rescore is not None:
        raise ValueError('a rescoring fit starts from the plain run with the consistency measures: consistency=True, no nms_iou, soft_nms, '
                         'min_* threshold or model')
    names_f = ordered(features) if features is not None else list(DEFAULT_FEATURES) + (['view_iou'] if detector.tta is not None else [])
    if 'view_iou' in names_f and detector.tta is None:
        raise ValueError('the feature view_iou is the agreement of the augmented views: it needs --tta')
    if isinstance(idx_list, str):
        idx_list = [int(line.rstrip()) for line in open(idx_list) if line.strip()]
    idx_list = [int(i) for i in idx_list]
    meta, d = detector.decode_all(parts)
    if d is None:
        raise ValueError('no detections to fit on')
    rt, stages = detector.rt, detector.stages
    n, names = len(meta), [m.name for m in meta]
    gt_all = ES.benchmark_groundtruth(dataset_dir, idx_list)
    with_gt = set(gt_all['classname'])
    if classes is None:
        classes = [c for c in ES.CLASS_NAMES[test_on] if c in with_gt and c in names]
    classes = list(classes)
    bad = [c for c in classes if c not in with_gt]
    if bad or not classes:
        raise ValueError('no ground truth among the images for the classes %s: nothing to fit on' % (bad or classes))
    held = ES.official_predictions(sorted(set(classes) | set(names)), detector.predictions(meta, d), names)
    rows_of = {c: np.nonzero(np.asarray([x == c for x in names], bool))[0] for c in classes}
    y, overlap = np.zeros(n, np.uint8), np.zeros(n)
    for c in classes:
        r = ES.compute_pr_curve_3d(c, held[c], gt_all, None, threshold, rt)
        ov = np.zeros(len(rows_of[c]))
        ov[r['sortIdx']] = r['maxOverlaps']                       # the script leaves them in sorted order
        overlap[rows_of[c]] = ov
        y[rows_of[c]] = (ov >= threshold) if target == 'overlap' else r['isTp']
    perm = np.random.RandomState(seed).permutation(len(idx_list))
    out_images = set(idx_list[k] for k in perm[:int(round(holdout * len(idx_list)))])
    in_classes = np.asarray([x in classes for x in names], bool)
    in_fit = np.asarray([m.image not in out_images for m in meta], bool)
    dr = DeviceRescore(rt, stages.n, names_f)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)
    pad = lambda a, dtype: np.concatenate([np.asarray(a, dtype), np.zeros(stages.n - n, dtype)])
    prob = np.asarray([m.prob for m in meta], np.float32)
    con, ens = stages.consistency, stages.ensemble_out
    dr.features(dev(pad(prob, np.float32)), stages.score, con.reproj, con.counts, None if ens is None else ens.agreement)
    dr.fit(dev(pad(y, np.uint8)), dev(pad((in_classes & in_fit).astype(np.float64), np.float64)), lam, max_iter=max_iter)
    dr.apply(n_valid=n)
    f = dr.fetch_fit()
    rescored = dr.out[:n].cpu().numpy()
    k = f['n_iter']
    log('rescore: fit on %d detections (%d positive) of %d classes, %d iterations, loss %s -> %s%s' % (
        f['n_rows'], f['n_pos'], len(classes), k, *(('%.6f' % f['loss'][0], '%.6f' % f['loss'][k - 1]) if k else ('-', '-')),
        ' [%s]' % ', '.join(status_names(f['status'])) if f['status'] else ''))
    log('rescore: coefficients per standardised feature: %s, intercept %.4f' % (
        ', '.join('%s %.4f' % kv for kv in zip(dr.names, f['coef_std'])), f['coef_std'][-1]))
    report = None
    if out_images:
        out_rows = in_classes & ~in_fit
        gt_out = ES.select_boxes(gt_all, np.asarray([int(i) in out_images for i in gt_all['image']], bool))
        report = {'images': len(out_images), 'detections': int(out_rows.sum()), 'classes': {}}
        for c in classes:
            sel = np.asarray([m.image in out_images for m in (meta[i] for i in rows_of[c])], bool)
            boxes = ES.select_boxes(held[c], sel)
            ap = {}
            for which, conf in (('prob', prob[rows_of[c]][sel].astype(np.float64)), ('rescore_prob', rescored[rows_of[c]][sel])):
                ap[which] = ES.compute_pr_curve_3d(c, dict(boxes, confidence=conf), gt_out, None, threshold, rt)['apScore']
            report['classes'][c] = {'detections': int(sel.sum()), 'ap_prob': ap['prob'], 'ap_rescore_prob': ap['rescore_prob']}
            log('rescore: held-out AP for %s: by prob %s, by rescore_prob %s' % (c.upper(), ES.num2str(100.0 * ap['prob']), ES.num2str(100.0 * ap['rescore_prob'])))
        for which in ('prob', 'rescore_prob'):
            report['mean_ap_' + which] = float(np.mean([v['ap_' + which] for v in report['classes'].values()]))
        report['log_loss_prob'], report['log_loss_rescore_prob'] = log_loss(prob[out_rows], y[out_rows]), log_loss(rescored[out_rows], y[out_rows])
        report['reliability'] = reliability(rescored[out_rows], y[out_rows])
        log('rescore: held-out mean AP: by prob %s, by rescore_prob %s' % (ES.num2str(100.0 * report['mean_ap_prob']),
                                                                           ES.num2str(100.0 * report['mean_ap_rescore_prob'])))
        if report['detections']:
            log('rescore: held-out log-loss: prob %.4f, rescore_prob %.4f' % (report['log_loss_prob'], report['log_loss_rescore_prob']))
            for b in report['reliability']:
                if b['n']:
                    log('rescore: reliability [%.1f, %.1f): %d detections, mean predicted %.3f, observed %.3f' % (
                        b['lo'], b['hi'], b['n'], b['mean_predicted'], b['observed']))
    model = Model(dr.names, f['coef'], f['coef_std'], f['mean'], f['scale'], target=target, threshold=threshold, lam=lam, classes=classes,
                  n_rows=f['n_rows'], n_pos=f['n_pos'], loss=f['loss'][k - 1] if k else None, status=status_names(f['status']), n_iter=k,
                  holdout=report)
    if path:
        model.save(path)
        log('rescoring model of %d features written to %s' % (len(dr.names), path))
    return model
