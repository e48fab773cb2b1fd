"""Sweep of the post-processing thresholds of `detect` against the official AP, on the device (detect --sweep, Detector.sweep).

--nms_iou and the three --min_* thresholds only choose which of the decoded detections are kept, so a grid over them needs one plain
run: the decoded corners, the consistency measures, what ranks and the (image, class) groups are all there afterwards.  Two entry
points score the whole grid from them:

    t3d_detect_nms_sweep      (nms.DeviceNmsSweep) the suppression of every configuration, each pair's IoU computed once;
    t3d_sunrgbd_eval_sweep    (evaluate_sunrgbd.sweep) per class the official evaluation of every configuration's detections, the
                              footprints, ranks and overlaps computed once.

A configuration is one value per flag, `off` among them; the grid is the product of the value lists in the order of FLAGS, the last
flag running fastest, `off` first in a list that has it.  The detections a configuration's --min_* values accept (consistency.accept_of's
rule: `~(v >= t)` rejects) are its `listed` row, built on the device; they are rejected before the suppression, as in `detect`.  The
`keep` matrix of the suppression goes to the evaluation as it lies, each class reading its own columns.

Box voting (--nms_fuse) moves the kept boxes, so its overlaps differ per configuration: it is not swept.
"""
import itertools
import json

import numpy as np
import torch

from . import abi, consistency as CS, evaluate_sunrgbd as ES, nms as NMS

FLAGS = ('nms_iou',) + CS.THRESHOLDS          # the order of the grid, and of a row's values


def add_arguments(parser):
    parser.add_argument('--sweep', action='store_true',
                        help='run once without thresholds, then score every combination of the --sweep_* values by the official AP on the device')
    for name in FLAGS:
        parser.add_argument('--sweep_' + name, nargs='+', default=None, metavar='V',
                            help='--sweep: the values of --%s to try, or the word off (default: off)' % name)
    parser.add_argument('--sweep_json', default=None, help='--sweep: write every row of the grid to this file')
    parser.add_argument('--sweep_top', type=int, default=None, help='--sweep: how many of the best rows are logged (default 10)')


def value_list(name, tokens):
    """The tokens of one --sweep_* flag (None: the flag was not given) -> its values, None standing for `off`: `off` first when
    present, every value once, otherwise in the order given."""
    if tokens is None:
        return [None]
    out, off = [], False
    for t in tokens:
        if t is None or (isinstance(t, str) and t.strip().lower() == 'off'):
            off = True
            continue
        try:
            v = float(t)
        except (TypeError, ValueError):
            raise ValueError('--sweep_%s takes numbers or the word off, got %r' % (name, t))
        if v not in out:
            out.append(v)
    return ([None] if off else []) + out


def flags_text(row):
    """The flags to pass for one row: '--nms_iou 0.25 --min_reproj_iou 0.5'; '(no flags)' where everything is off."""
    parts = ['--%s %g' % (name, v) for name, v in zip(FLAGS, row) if v is not None]
    return ' '.join(parts) if parts else '(no flags)'


class Grid:
    """The configurations of a sweep.  Each of nms_iou, min_reproj_iou, min_mask_in_box, min_seg_box_iou: None (not swept: off), or a
    list of values the flag of that name accepts and / or 'off'.  nms_metric / nms_score hold for every configuration."""

    def __init__(self, nms_iou=None, min_reproj_iou=None, min_mask_in_box=None, min_seg_box_iou=None, nms_metric=None, nms_score=None):
        given = dict(zip(FLAGS, (nms_iou, min_reproj_iou, min_mask_in_box, min_seg_box_iou)))
        if all(v is None for v in given.values()):
            raise ValueError('--sweep needs at least one of ' + ' '.join('--sweep_' + f for f in FLAGS))
        self.values = {name: value_list(name, tokens) for name, tokens in given.items()}
        self.thresholds = [v for v in self.values['nms_iou'] if v is not None]      # the distinct NMS thresholds, in grid order
        for v in self.thresholds:
            NMS.check_options(v, nms_metric, nms_score)
        if not self.thresholds and (nms_metric is not None or nms_score is not None):
            raise ValueError('--nms_metric / --nms_score need a value of --sweep_nms_iou')
        self.metric, self.score = nms_metric or '3d', nms_score or 'prob'
        for k, name in enumerate(CS.THRESHOLDS):
            for v in self.values[name]:
                CS.check_thresholds(*[v if j == k else None for j in range(3)])
        if len(self.thresholds) > abi.NMS_SWEEP_MAX_THRESHOLDS:
            raise ValueError('%d distinct values of --sweep_nms_iou: one sweep takes %d' % (len(self.thresholds), abi.NMS_SWEEP_MAX_THRESHOLDS))
        M = int(np.prod([len(self.values[f]) for f in FLAGS], dtype=np.int64))
        if M > abi.SWEEP_MAX_CONFIGS:
            raise ValueError('%d configurations: one sweep takes %d' % (M, abi.SWEEP_MAX_CONFIGS))
        self.rows = list(itertools.product(*[self.values[f] for f in FLAGS]))
        self.consistency = any(given[name] is not None for name in CS.THRESHOLDS)      # the measures are taken iff a --sweep_min_* is given

    def __len__(self):
        return len(self.rows)

    @classmethod
    def from_args(cls, args):
        return cls(args.sweep_nms_iou, args.sweep_min_reproj_iou, args.sweep_min_mask_in_box, args.sweep_min_seg_box_iou,
                   args.nms_metric, args.nms_score)


def device_listed(rt, rows, measures, n):
    """listed uint8 [len(rows), n] on the runtime's device: which detections the --min_* values of each row accept, by
    consistency.accept_of's rule; None where no row has such a value.  measures: {name of consistency.MEASURES: fp64 [n]}."""
    listed = None
    for j, (name, measure) in enumerate(zip(CS.THRESHOLDS, CS.MEASURES)):
        col = [r[1 + j] for r in rows]
        if all(v is None for v in col):
            continue
        if listed is None:
            listed = torch.ones(len(rows), n, dtype=torch.bool, device=rt.device)
        t = torch.tensor([0.0 if v is None else v for v in col], dtype=torch.float64, device=rt.device)
        on = torch.tensor([v is not None for v in col], dtype=torch.bool, device=rt.device)
        v = torch.from_numpy(np.ascontiguousarray(measures[measure], np.float64)).to(rt.device)
        bad = ~(v[None, :] >= t[:, None])
        listed &= ~(bad & on[:, None])
    return None if listed is None else listed.to(torch.uint8).contiguous()


class Result:
    """What a sweep found.  rows: the grid's rows (tuples in FLAGS order); ap {class: float64 [M]}, n_det / n_tp / n_fp {class: int32
    [M]}, mean_ap float64 [M], kept int [M]: the detections each configuration keeps, of all classes; baseline: the same numbers of the
    configuration with everything off (which the grid need not hold)."""

    def __init__(self, grid, classes, per_class, mean_ap, kept, n_detections, base, test_on, threshold):
        M = len(grid)
        self.grid, self.rows, self.classes, self.n_detections, self.test_on, self.threshold = grid, grid.rows, list(classes), n_detections, test_on, threshold
        self.baseline = self._row(base, (None,) * len(FLAGS), per_class, mean_ap, kept)
        self.ap = {c: per_class[c]['ap'][:M] for c in classes}
        self.n_det, self.n_tp, self.n_fp = ({c: per_class[c][k][:M] for c in classes} for k in ('n_det', 'n_tp', 'n_fp'))
        self.mean_ap, self.kept = mean_ap[:M], kept[:M]
        self._table = [self._row(m, self.rows[m], per_class, mean_ap, kept) for m in range(M)]
        self.bootstrap = None          # set by `bootstrap_rows`

    def _row(self, m, row, per_class, mean_ap, kept):
        return {'index': int(m), 'options': dict(zip(FLAGS, row)), 'flags': flags_text(row), 'mean_ap': float(mean_ap[m]),
                'ap': {c: float(per_class[c]['ap'][m]) for c in self.classes}, 'kept': int(kept[m]),
                'n_det': {c: int(per_class[c]['n_det'][m]) for c in self.classes}, 'n_tp': {c: int(per_class[c]['n_tp'][m]) for c in self.classes},
                'n_fp': {c: int(per_class[c]['n_fp'][m]) for c in self.classes}}

    def table(self):
        """One dictionary per row of the grid, in grid order."""
        return self._table

    def ranking(self, top=None):
        """The rows' indices, best mean AP first, ties in grid order."""
        order = sorted(range(len(self.rows)), key=lambda m: (-self.mean_ap[m], m))
        return order if top is None else order[:max(int(top), 0)]

    def best(self):
        return self._table[self.ranking(1)[0]]

    def _text(self, r):
        return 'mAP %s | %s | kept %d' % (ES.num2str(r['mean_ap'] * 100.0), ' '.join('%s %.2f' % (c, 100.0 * r['ap'][c]) for c in self.classes), r['kept'])

    def lines(self, top=10):
        out = ['sweep: %d configurations over %d detections of %d classes' % (len(self.rows), self.n_detections, len(self.classes)),
               'baseline: ' + self._text(self.baseline)]
        boot = self.bootstrap
        for k, m in enumerate(self.ranking(top)):
            text = self._text(self._table[m])
            if boot is not None and m in boot['rows']:
                from . import bootstrap as BS
                text += ' | vs baseline %s | vs best %s' % (BS.difference_text(boot['rows'][m]['vs_baseline']), BS.difference_text(boot['rows'][m]['vs_best']))
            out.append('%3d. %s: %s' % (k + 1, self._table[m]['flags'], text))
        out.append('best: ' + self.best()['flags'])
        if boot is not None:
            same = [k + 1 for k, m in enumerate(self.ranking(top)) if k > 0 and m in boot['rows']
                    and boot['rows'][m]['vs_best']['lo'] <= 0.0 <= boot['rows'][m]['vs_best']['hi']]
            out.append('indistinguishable from best at %g %%: %s' % (round(100.0 * boot['level'], 10),
                                                                     'rows ' + ', '.join(str(k) for k in same) if same else 'none'))
        return out

    def bootstrap_rows(self, rt, top, keep, predictions, det_index, gt_all, idx_list, options):
        """The paired bootstrap of the `top` best rows (options: {'R', 'seed', 'level'}; bootstrap.py): per row, evaluate_sunrgbd.
        bootstrap_class per class on the detections its row of `keep` selects, with one weight matrix for all rows, so that per
        replicate the mean AP of two rows can be subtracted.  Every such row of `table()` gains 'bootstrap': {'mean_ap': the summary of
        its replicate mean APs, 'vs_baseline': the row minus the baseline, 'vs_best': the row minus the best row (mean, se, lo, hi,
        p_le0)}.  Rows outside the list are not bootstrapped."""
        from . import bootstrap as BS
        level = options.get('level', 0.95)
        weights = options.get('weights') or BS.Weights(rt, len(idx_list), options['R'], options.get('seed', 0))
        ranked = self.ranking(top)
        best, base = self.ranking(1)[0], self.baseline['index']

        def replicates(m):
            row = keep[m].cpu().numpy()
            ap = {}
            for c in self.classes:
                cols = np.arange(len(predictions[c]['confidence'])) if det_index.get(c) is None else np.asarray(det_index[c], np.int64)
                ok = (cols >= 0) & (cols < len(row))
                sel = np.zeros(len(cols), bool)
                sel[ok] = row[cols[ok]] != 0
                ap[c] = ES.bootstrap_class(c, ES.select_boxes(predictions[c], sel), gt_all, weights, idx_list, self.threshold, rt)['ap']
            return BS.mean_over_classes(ap)
        vec = {m: replicates(m) for m in dict.fromkeys(ranked + [best, base])}
        rows = {m: {'mean_ap': BS.summary({'mean': vec[m]}, level)['mean_ap'], 'vs_baseline': BS.paired_vector(vec[base], vec[m], level),
                    'vs_best': BS.paired_vector(vec[best], vec[m], level)} for m in ranked}
        self.bootstrap = {'R': weights.R, 'seed': weights.seed, 'level': level, 'rows': rows, 'replicates': vec}
        for m, r in rows.items():
            self._table[m]['bootstrap'] = r
        return self.bootstrap

    def write_json(self, path):
        with open(path, 'w') as fh:
            json.dump({'test_on': self.test_on, 'threshold': self.threshold, 'nms_metric': self.grid.metric, 'nms_score': self.grid.score,
                       'flags': list(FLAGS), 'values': self.grid.values, 'classes': self.classes, 'detections': self.n_detections,
                       'baseline': self.baseline, 'best': self.best(), 'rows': self._table,
                       **({} if self.bootstrap is None else {'bootstrap': {k: self.bootstrap[k] for k in ('R', 'seed', 'level')}})}, fh, indent=1)


def run(rt, grid, corners, score, image_ids, class_ids, measures, predictions, det_index, dataset_dir, idx_list, test_on='AB', threshold=0.25,
        gt_all=None, bootstrap=None, top=10):
    """corners [n, 24] and score [n] fp32 on the runtime's device (what t3d_detect_decode wrote, and what ranks); image_ids, class_ids [n]:
    the groups; measures: {reproj_iou, mask_in_box, seg_box_iou: fp64 [n]} of the run, or None when grid.consistency is False;
    predictions {class: boxes} and det_index {class: the detections of the class among the n, ascending}: what evaluate_sunrgbd.sweep
    takes.  bootstrap: None, or {'R', 'seed', 'level'}: Result.bootstrap_rows for the `top` best rows.  -> Result."""
    if bootstrap is not None:
        if isinstance(idx_list, str):
            idx_list = [int(line.rstrip()) for line in open(idx_list) if line.strip()]
        idx_list = list(idx_list)
        if gt_all is None:
            gt_all = ES.benchmark_groundtruth(dataset_dir, idx_list)
    rows = list(grid.rows)
    off = (None,) * len(FLAGS)
    if off in rows:
        base = rows.index(off)
    else:                                                    # the baseline row travels behind the grid's
        base = len(rows)
        rows.append(off)
        if len(rows) > abi.SWEEP_MAX_CONFIGS:
            raise ValueError('%d configurations and the baseline: one sweep takes %d' % (len(grid), abi.SWEEP_MAX_CONFIGS))
    n = len(image_ids)
    offsets, members = NMS.groups_of(image_ids, class_ids)
    thresholds = grid.thresholds or [1.0]                    # (no threshold is swept: every configuration names -1)
    ct = np.asarray([-1 if r[0] is None else thresholds.index(r[0]) for r in rows], np.int32)
    listed = device_listed(rt, rows, measures, n) if grid.consistency else None
    dev = NMS.DeviceNmsSweep(rt)
    keep, n_kept = dev.run(corners, score, offsets, members, thresholds, ct, listed, grid.metric)
    per_class, mean_ap = ES.sweep(predictions, dataset_dir, idx_list, keep, det_index, test_on, rt, threshold, gt_all)
    result = Result(grid, ES.CLASS_NAMES[test_on], per_class, mean_ap, n_kept.cpu().numpy().astype(np.int64), n, base, test_on, threshold)
    if bootstrap is not None:
        result.bootstrap_rows(rt, top, keep, predictions, det_index, gt_all, idx_list, bootstrap)
    return result
