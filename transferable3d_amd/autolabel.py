#!/usr/bin/env python3
"""3-D labels for classes that have 2-D labels only: a trained model plus 2-D boxes in, a `label_dimension` data set out.

    python -m transferable3d_amd.autolabel --dataset_dir D --idx_path I --classes table sofa dresser night_stand bookshelf \
        --model_path M [test_semisup's model flags] --out_dir OUT [--min_reproj_iou T] [--min_mask_in_box F] [--min_seg_box_iou F] \
        [--keep_other_classes] [--link_inputs] [--score_against_labels] [--tta K [--tta_flip] [--tta_vote_iou V] [--min_view_iou A]] \
        [--rescore MODEL.json [--min_rescore P]] [--floor] [--snap_floor {shift,stretch} [--snap_floor_max M]] [--max_floor_gap G] \
        [--floor_json FILE] [--floor_bin B] [--floor_range LO HI] [--floor_min_share F] [--floor_band D] [--floor_max_tilt DEG] \
        [--visibility] [--visibility_cell PX] [--visibility_margin M] [--visibility_min_chord M] [--max_see_through F \
        [--visibility_min_rays N]]

Of every object of --classes in D/training/label_dimension/*.txt only the class and the 2-D box are used.  detect.Detector runs on that
box (with prob 1); t3d_detect_consistency (consistency.py) measures the 3-D box it predicts against the 2-D box and the segmented points,
and the thresholds accept or reject it.  The accepted boxes are written as label lines, in the toolbox's format, to
OUT/training/label_dimension/%06d.txt; OUT/training/autolabel_idx.txt lists the scenes with at least one line, OUT/autolabel.json the
counts per class (offered, too few points, accepted, rejected by each test).  With --keep_other_classes the lines of all other classes
are copied unchanged; with --link_inputs the image, calib and depth folders of D/training are linked into OUT/training, so that OUT is
a data set root for sunrgbd_data and evaluate_sunrgbd.

--score_against_labels: where the label lines do carry a 3-D box (strong classes), report per class, for accepted and rejected boxes
separately, the mean 3-D IoU (t3d_box3d_iou_corners) with the label's own box and the share at IoU >= 0.25 -- to set the thresholds on
classes with 3-D labels before applying them to classes without.

--tta K [--tta_flip] [--tta_vote_iou V] [--min_view_iou A]: detect's test-time augmentation (ensemble.py).  Every object is predicted in K
views, the label line is written from their fused box, and --min_view_iou rejects a box whose views overlap by less than A on average
-- stability under augmentation, the one test here that does not compare the box with its own frustum.  --score_against_labels then
reports the accepted and the rejected boxes of that test alone as well.

--rescore MODEL.json [--min_rescore P]: detect's rescoring (rescore.py).  A model fitted by `detect --rescore_fit` on the classes with 3-D
labels gives every box one confidence from its measures, and --min_rescore rejects a box below P: one calibrated accept rule in the
place of three cut-offs picked by hand (they still combine).  Every object is offered with prob 1, so a model's logit_prob column is
constant here.  --score_against_labels reports the boxes that test alone accepts and rejects as well.

--floor, --snap_floor, --max_floor_gap and the estimator's flags: detect's floor stage (floor.py).  The label line is written from the
snapped box, --max_floor_gap rejects a box that floats above or sinks into its scene's floor by more than G, and
--score_against_labels reports the boxes that test alone accepts and rejects as well.

--visibility, --max_see_through and their flags: detect's visibility stage (visibility.py).  --max_see_through rejects a box through
which the scene behind it is seen (on at least --visibility_min_rays rays), and --score_against_labels reports the boxes that test
alone accepts and rejects as well.

A label line, from a decoded label row (h, w, l, tx, ty, tz, ry) (`label_line`): the 2-D box as x, y, w, h; the centroid (tx, tz,
-(ty - h/2)) in upright depth coordinates; the half sizes (w/2, l/2, h/2); the basis (cos ry, -sin ry, sin ry, cos ry); the orientation
(cos ry, -sin ry).  sunrgbd_data.SUNObject3d + compute_box_3d read such a line back as the decode's corner set, to the six decimals of %f.
"""
import argparse
import collections
import json
import os
import sys

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transferable3d_amd import consistency as CS, ensemble as EN, floor as FL, rescore as RS, semisup_infer as SI, sunrgbd_data as SD, test_semisup as TS, visibility as VS      # noqa: E402

LINE = '%s %d %d %d %d %f %f %f %f %f %f %f %f %f %f %f %f'
IOU_HIT = 0.25


def label_line(classname, box2d, label):
    """One label_dimension line of a decoded label row (h, w, l, tx, ty, tz, ry); box2d = (xmin, ymin, xmax, ymax)."""
    h, w, l, tx, ty, tz, ry = [float(v) for v in label]
    x0, y0, x1, y1 = [float(v) for v in box2d]
    c, s = np.cos(ry), np.sin(ry)
    return LINE % (classname, round(x0), round(y0), round(x1 - x0), round(y1 - y0), tx, tz, -(ty - h / 2.0), w / 2.0, l / 2.0, h / 2.0,
                   c, -s, s, c, c, -s)


def label_corners(obj):
    """The 3-D box of a label line as 8 corners in upright camera coordinates, in get_3d_box order (what t3d_box3d_iou_corners takes)."""
    from transferable3d_amd.eval_det import get_3d_box
    return get_3d_box((2.0 * obj.l, 2.0 * obj.w, 2.0 * obj.h), obj.heading_angle, (obj.centroid[0], -obj.centroid[2], obj.centroid[1]))


def rejected_by(tests, rows):
    """{flag: [len(rows)] bool} of the active tests (semisup_infer.active_tests), in their order: which of the records `rows` each
    test alone rejects -- the predicates of semisup_infer.TESTS on arrays made of the records' fields."""
    return collections.OrderedDict((t.flag, t.rejected(*(np.array([r[k] for r in rows]) for k in t.fields), limit, **parameters))
                                   for t, limit, parameters in tests)


def new_counts(tests):
    c = collections.OrderedDict(offered=0, too_few_points=0, accepted=0, rejected=0)
    c['rejected_by'] = collections.OrderedDict((t.flag, 0) for t, _, _ in tests)
    return c


def count(records, classes, tests):
    """records: [{'class', 'detected' (False: its frustum held too few points), 'accepted', and the fields the tests read}]; tests: the
    active tests (semisup_infer.active_tests) -> {class: offered, too_few_points, accepted, rejected, rejected_by {flag: n}} (a box may
    fail several tests)."""
    out = collections.OrderedDict((c, new_counts(tests)) for c in classes)
    rows = [r for r in records if r['detected']]
    for r in records:
        out[r['class']]['offered'] += 1
        out[r['class']]['too_few_points'] += not r['detected']
    for r in rows:
        out[r['class']]['accepted' if r['accepted'] else 'rejected'] += 1
    for flag, bad in rejected_by(tests, rows).items():
        for r in np.array(rows, object)[bad]:
            out[r['class']]['rejected_by'][flag] += 1
    return out


def score(records, classes, rt, tests):
    """--score_against_labels: per class, for the accepted and the rejected boxes, how many, their mean 3-D IoU with the label's own box
    and the share at IoU >= 0.25; and the same under its flag for the boxes each of the active tests (semisup_infer.active_tests)
    beside the consistency thresholds alone accepts and rejects."""
    from transferable3d_amd.eval_det import box3d_iou_batch
    rows = [r for r in records if r['detected']]
    iou = np.asarray(box3d_iou_batch(np.stack([r['corners'] for r in rows]), np.stack([r['label_corners'] for r in rows]), rt)[0] if rows else [], np.float64)
    names = np.array([r['class'] for r in rows], object)
    kinds = collections.OrderedDict(accepted=np.array([r['accepted'] for r in rows], bool))
    kinds.update((flag, ~bad) for flag, bad in rejected_by([t for t in tests if t[0] not in CS.TESTS], rows).items())
    stats = lambda v: {'n': len(v), 'mean_iou3d': float(v.mean()) if len(v) else None,
                       'share_iou_ge_0.25': float((v >= IOU_HIT).mean()) if len(v) else None}
    out = collections.OrderedDict()
    for c in classes:
        by = {key: {kind: stats(iou[(names == c) & (ok == (kind == 'accepted'))]) for kind in ('accepted', 'rejected')} for key, ok in kinds.items()}
        out[c] = dict(by.pop('accepted'), **by)          # 'accepted' and 'rejected' of the run itself, then of each test under its flag
    return out


def run(detector, dataset_dir, ids, classes, out_dir, keep_other_classes=False, link_inputs=False, score_against_labels=False, log=print,
        batch_scenes=16, workers=8, floor_json=None):
    """The command (module text) with a detect.Detector built by the caller (its thresholds decide).  ids: scene ids, or the path of an
    index file.  -> the dict written to OUT/autolabel.json, plus '_records': one entry per offered object (not written)."""
    from transferable3d_amd.detect import consistency_fields, scene_batches, view_fields, visibility_fields
    if isinstance(ids, str):
        ids = [int(line.rstrip()) for line in open(ids) if line.strip()]
    classes = list(classes)
    bad = [c for c in classes if c not in detector.whitelist or (detector.classes is not None and c not in detector.classes)]
    if bad:
        raise ValueError('the detector does not take the classes %s (its whitelist / SUNRGBD_SEMI_TEST_CLS)' % bad)
    dataset = SD.sunrgbd_object(dataset_dir, 'training')
    lines = {}

    def read_lines(idx):
        with open(dataset._path('label_dimension', idx, 'txt')) as fh:
            lines[idx] = [line.rstrip() for line in fh if line.strip()]

    floor, visibility = detector.floor, detector.visibility
    image_wh = (lambda path: CS.image_size(path) if os.path.exists(path) else None) if detector.consistency or visibility.on else None
    parts, offered = [], []
    for batch, scenes in scene_batches(dataset, ids, batch_scenes, workers, image_wh=image_wh, also=read_lines):
        dets = []
        for idx in batch:
            take = [(k, o) for k, o in enumerate(SD.SUNObject3d(line) for line in lines[idx]) if o.classname in classes]
            dets.append([(o.classname, o.box2d, 1.0) for _, o in take])
            offered.append((idx, take))
        parts.append(detector.extract(scenes, dets, batch))
    if floor_json:
        FL.write_json(floor_json, detector.floor_json_rows(parts))
    meta, d = detector.decode_all(parts)
    # the detections come back in the order they were offered, without those whose frustum held too few points
    records, i = [], 0
    for idx, take in offered:
        for k, o in take:
            hit = i < len(meta) and meta[i].image == idx and meta[i].name == o.classname and np.array_equal(meta[i].box2d, o.box2d)
            r = {'image': idx, 'line': k, 'class': o.classname, 'box2d': o.box2d, 'detected': bool(hit), 'accepted': False}
            if hit:
                r.update(accepted=bool(d.keep is None or d.keep[i]), label=d.label[i], corners=d.corners[i], row=i)
                if d.reproj_iou is not None:
                    fields = consistency_fields(d, i)
                    r.update((k, fields[k]) for k in CS.MEASURES + ('flags',))
                if d.view_iou is not None:
                    r.update(view_fields(d, i))
                if d.rescore_prob is not None:
                    r['rescore_prob'] = float(d.rescore_prob[i])
                if d.floor_gap is not None:
                    r.update(floor_gap=float(d.floor_gap[i]), floor_flags=int(d.floor_flags[i]))
                if d.see_through is not None:
                    r.update(visibility_fields(d, i), visibility_evidence=int(VS.evidence(d.visibility_profile[i])))
                if score_against_labels:
                    r['label_corners'] = label_corners(o)
                i += 1
            records.append(r)
    assert i == len(meta), 'a detection matches no offered object'
    tests = SI.active_tests(detector, floor, visibility)
    summary = collections.OrderedDict(classes=count(records, classes, tests), thresholds=dict(zip(CS.THRESHOLDS, detector.thresholds)), scenes=len(ids))
    if detector.tta is not None:
        summary['tta'] = dict(views=detector.tta, flip=detector.tta_flip, vote_iou=detector.tta_vote_iou, min_view_iou=detector.min_view_iou)
    if detector.rescore is not None:
        summary['rescore'] = dict(features=detector.rescore.features, min_rescore=detector.min_rescore)
    if floor.on:
        summary['floor'] = dict(snap=floor.snap, snap_max=floor.snap_max, max_floor_gap=floor.max_floor_gap)
    if visibility.on:
        o = visibility.options
        summary['visibility'] = dict(cell=o.cell, margin=o.margin, min_chord=o.min_chord, max_see_through=visibility.max_see_through, min_rays=o.min_rays)
    if score_against_labels:
        summary['score_against_labels'] = score(records, classes, detector.rt, tests)
    written = write_labels(out_dir, ids, lines, records, classes, keep_other_classes)
    summary['scenes_written'] = len(written)
    if link_inputs:
        link(dataset.split_dir, os.path.join(out_dir, 'training'))
    with open(os.path.join(out_dir, 'autolabel.json'), 'w') as fh:
        json.dump(summary, fh, indent=1)
    for c, n in summary['classes'].items():
        log('%s: offered %d, too few points %d, accepted %d, rejected %d%s' % (
            c, n['offered'], n['too_few_points'], n['accepted'], n['rejected'],
            ''.join(' (%s: %d)' % kv for kv in n['rejected_by'].items())))
        if score_against_labels:
            by = summary['score_against_labels'][c]
            for kind, v in [(k, by[k]) for k in ('accepted', 'rejected')] + [('%s by --%s' % (k, flag), v) for flag in list(by)[2:] for k, v in by[flag].items()]:
                if v['n']:
                    log('  %s %d: mean 3-D IoU with the label %.3f, at IoU >= %g %.1f %%' % (kind, v['n'], v['mean_iou3d'], IOU_HIT,
                                                                                            100.0 * v['share_iou_ge_0.25']))
    log('%d label files written to %s' % (len(written), os.path.join(out_dir, 'training', 'label_dimension')))
    summary['_records'] = records
    return summary


def write_labels(out_dir, ids, lines, records, classes, keep_other_classes):
    """OUT/training/label_dimension/%06d.txt (the lines of a scene in their original order: an accepted object's new line, another
    class's line as it stood) and OUT/training/autolabel_idx.txt.  -> the ids of the scenes with at least one line."""
    folder = os.path.join(out_dir, 'training', 'label_dimension')
    os.makedirs(folder, exist_ok=True)
    new = {(r['image'], r['line']): label_line(r['class'], r['box2d'], r['label']) for r in records if r['accepted']}
    written = []
    for idx in ids:
        out = []
        for k, line in enumerate(lines[idx]):
            if line.split(' ', 1)[0] in classes:
                if (idx, k) in new:
                    out.append(new[(idx, k)])
            elif keep_other_classes:
                out.append(line)
        if out:
            with open(os.path.join(folder, '%06d.txt' % idx), 'w') as fh:
                fh.write(''.join(l + '\n' for l in out))
            written.append(idx)
    with open(os.path.join(out_dir, 'training', 'autolabel_idx.txt'), 'w') as fh:
        fh.write(''.join('%d\n' % i for i in written))
    return written


def link(src_split, dst_split):
    for sub in ('image', 'calib', 'depth'):
        src, dst = os.path.abspath(os.path.join(src_split, sub)), os.path.join(dst_split, sub)
        if os.path.isdir(src) and not os.path.lexists(dst):
            os.symlink(src, dst)


def parser():
    p = argparse.ArgumentParser(description='3-D label files for classes with 2-D labels, from a trained model', allow_abbrev=False)
    p.add_argument('--dataset_dir', default='mysunrgbd', help='SUN-RGBD root (<dir>/training/{image,calib,depth,label_dimension})')
    p.add_argument('--idx_path', required=True, help='index file of the scenes to label')
    p.add_argument('--classes', nargs='+', required=True, help='classes whose objects get a 3-D box from their 2-D box')
    p.add_argument('--out_dir', required=True, help='root of the data set to write (<out_dir>/training/label_dimension/%%06d.txt)')
    for name, what in zip(CS.THRESHOLDS, ('reprojection IoU', 'share of segmented points inside the box', 'IoU of segmented points and points inside the box')):
        p.add_argument('--' + name, type=float, default=None, help='reject a box whose %s lies below this (0..1)' % what)
    p.add_argument('--keep_other_classes', action='store_true', help='copy the label lines of all other classes unchanged')
    p.add_argument('--link_inputs', action='store_true', help='link image, calib and depth of the data set into <out_dir>/training')
    p.add_argument('--score_against_labels', action='store_true', help='report the 3-D IoU of accepted and rejected boxes with the 3-D boxes of the label lines')
    EN.add_arguments(p)
    RS.add_arguments(p)
    FL.add_arguments(p)
    p.add_argument('--floor_json', default=None, help='write one row per scene with its floor plane, the share of its points on it, their rms and the flags here')
    VS.add_arguments(p)
    return p


def parse(argv=None):
    """-> (this module's arguments, test_semisup's FLAGS of everything else); a threshold outside [0, 1] is an argument error."""
    p = parser()
    args, rest = p.parse_known_args(argv)
    try:
        args.thresholds = CS.check_thresholds(args.min_reproj_iou, args.min_mask_in_box, args.min_seg_box_iou)
        EN.check_options(args.tta, args.tta_flip, args.tta_vote_iou, args.min_view_iou)
        if RS.check_min_rescore(args.min_rescore) is not None and args.rescore is None:
            raise ValueError('--min_rescore rejects by the rescored confidence: it needs --rescore')
        if args.floor_json and not FL.check_options(**{k: getattr(args, k) for k in FL.FLAGS}).on:
            raise ValueError('--floor_json writes the floor planes: it needs --floor, --snap_floor or --max_floor_gap')
        VS.check_options(**{k: getattr(args, k) for k in VS.FLAGS})
    except ValueError as e:
        p.error(str(e))
    return args, TS.build_flags(list(rest))


def main(argv=None, rt=None, log=print):
    from transferable3d_amd.detect import Detector
    args, FLAGS = parse(argv)
    if any(c not in FLAGS.SUNRGBD_SEMI_TEST_CLS for c in args.classes):      # (the flag only selects the classes the detector takes)
        FLAGS.SUNRGBD_SEMI_TEST_CLS = list(args.classes)
    det = Detector(FLAGS, rt=rt, log=log, consistency=True, min_reproj_iou=args.thresholds[0], min_mask_in_box=args.thresholds[1],
                   min_seg_box_iou=args.thresholds[2], tta=args.tta, tta_flip=args.tta_flip, tta_vote_iou=args.tta_vote_iou,
                   min_view_iou=args.min_view_iou, rescore=args.rescore, min_rescore=args.min_rescore,
                   **{k: getattr(args, k) for k in FL.FLAGS + VS.FLAGS})
    return run(det, args.dataset_dir, args.idx_path, args.classes, args.out_dir, keep_other_classes=args.keep_other_classes,
               link_inputs=args.link_inputs, score_against_labels=args.score_against_labels, log=log, floor_json=args.floor_json)


if __name__ == '__main__':
    main()
