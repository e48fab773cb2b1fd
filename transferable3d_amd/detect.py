#!/usr/bin/env python3
"""Scenes and 2-D detections in, 3-D boxes out, in one process and without a frustum file.

    python -m transferable3d_amd.detect --dataset_dir D --idx_path I --rgb_detection_path DETS --model_path M [--boxpc_model_path P] \
        --result_dir R [--official_eval]       # + test_semisup's model flags (--semi_type, --refine, --pred_prefix, --num_point, ...)
        [--nms_iou T [--nms_metric {3d,bev}] [--nms_score {prob,score}]]

What `sunrgbd_data --option rgb_detection` followed by `semisup_infer --from_rgb_detection --device_decode` computes, with the frustum
points staying where t3d_frustum_extract wrote them: extraction -> DeviceFrustumSet.from_device -> DeviceEvalSource -> the network ->
t3d_detect_decode.  Two things cross to the host: the per-job point counts of every extraction launch (the reference drops a frustum
of fewer than 5 points, sunrgbd_data.py:313-315) and the decoded records at the end.

As in test_semisup, a frustum's N points are drawn by a hash of (seed, batch, slot): its boxes depend on its position among the
frustums of the call.  One call over the scenes of a run therefore equals the two-step route over the same detections, and a call over
a part of them does not.

--nms_iou T: a 2-D detector reports one object several times, every report becomes a 3-D box, and the evaluation counts all but one of
them as false positives.  With the flag, t3d_detect_nms (nms.py) suppresses, per image and class, every box whose IoU with a
better-ranked kept box exceeds T, on the decoded corners where they lie; the suppressed detections are absent from everything this
module hands out.  Without it nothing changes.
"""
import argparse
import collections
import os
import sys

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transferable3d_amd import nms as NMS, semisup_infer as SI, sunrgbd_data as SD, test_semisup as TS      # noqa: E402
from transferable3d_amd.constants import type2class                        # noqa: E402
from transferable3d_amd.dataset import DeviceEvalSource, DeviceFrustumSet   # noqa: E402
from transferable3d_amd.tf_checkpoint import load_state                    # noqa: E402

MIN_POINTS = 5


def flags_from_keywords(**kw):
    """test_semisup's FLAGS from keyword arguments: semi_type='F', refine=1, use_one_hot=True, SUNRGBD_SEMI_TEST_CLS=[...], ..."""
    argv = []
    for k, v in kw.items():
        if isinstance(v, bool):
            argv += ['--' + k] if v else []
        elif isinstance(v, (list, tuple)):
            argv += ['--' + k] + [str(x) for x in v]
        elif v is not None:
            argv += ['--' + k, str(v)]
    return TS.build_flags(argv)


class Detector:
    """The test_semisup inference graph, built once; `detect` runs scenes through it."""

    def __init__(self, FLAGS=None, model_path=None, boxpc_model_path=None, rt=None, type_whitelist=SD.TYPE_WHITELIST,
                 num_points=SD.NUM_POINTS, nms_iou=None, nms_metric=None, nms_score=None, log=None, **keywords):
        """FLAGS: test_semisup.build_flags(...), or keyword arguments of the same names.  model_path / boxpc_model_path: state dicts
        (.npz) or TensorFlow checkpoint prefixes (default: FLAGS'; neither: the graph's initial weights).  num_points: the cap of a
        frustum's points at extraction (the frustum files': 2048); the network draws FLAGS.num_point of them per batch.
        nms_iou: None (every detection is reported, as the reference does) or the IoU in (0, 1] above which a box is suppressed by a
        better-ranked kept box of its image and class; nms_metric '3d' (default) / 'bev'; nms_score 'prob' (default: the 2-D
        detection confidence, what the result files and the evaluation rank by) / 'score' (the decoded network score).  log: a
        function that takes the one line per run on how many detections were kept."""
        self.nms_iou, self.nms_metric, self.nms_score = NMS.check_options(nms_iou, nms_metric, nms_score)
        self.log = log
        self.FLAGS = FLAGS = FLAGS if FLAGS is not None else flags_from_keywords(**keywords)
        model_path = model_path or FLAGS.model_path
        boxpc_model_path = boxpc_model_path or FLAGS.boxpc_model_path
        sd = load_state(model_path) if model_path else None
        if boxpc_model_path:
            sd = dict(sd or {})
            sd.update({'D_boxpc_branch/' + k: v for k, v in load_state(boxpc_model_path).items()})
        self.B = FLAGS.batch_size
        self.sess, self.ops = TS.get_model(FLAGS, self.B, FLAGS.num_point, FLAGS.NUM_CHANNELS, rt=rt, state_dict=sd)
        self.rt = self.ops['graph'].rt
        self.extractor = SD.FrustumExtractor(self.rt, num_points, FLAGS.seed)
        self.whitelist = list(type_whitelist)
        self.classes = list(FLAGS.SUNRGBD_SEMI_TEST_CLS) or None

    def extract(self, scenes, detections, scene_ids=None):
        """One t3d_frustum_extract launch over `scenes`; -> a part for `decode` (device tensors + what the host knows of the kept jobs)."""
        scene_ids = list(range(len(scenes))) if scene_ids is None else list(scene_ids)
        jobs, meta = [], []
        for s, dets in enumerate(detections):
            for o, (name, box2d, prob) in enumerate(dets):          # the ordinal counts every detection of the image (sunrgbd_data)
                if name not in self.whitelist or (self.classes is not None and name not in self.classes):
                    continue
                jobs.append({'scene': s, 'box2d': np.asarray(box2d, np.float64), 'box3d': None, 'key': (scene_ids[s], o, 0), 'choice': None})
                meta.append((s, scene_ids[s], name, np.asarray(box2d, np.float64), float(prob)))
        out = self.extractor.run(scenes, jobs, on_device=True)
        if out is None:
            return dict(out=None, keep=[], counts=[], meta=[], n_scenes=len(scenes))
        counts = out['count'].cpu().numpy()                          # the one copy back of this launch
        keep = np.nonzero(counts >= MIN_POINTS)[0]
        return dict(out=out, keep=keep, counts=counts[keep], meta=[meta[j] for j in keep], n_scenes=len(scenes))

    def decode(self, parts):
        """The network and t3d_detect_decode over the frustums of `parts` (in order) -> (meta, semisup_infer.Decoded); with nms_iou, of
        the detections t3d_detect_nms kept."""
        meta, d = self.decode_all(parts)
        if d is None or d.keep is None:
            return meta, d
        rows = np.nonzero(d.keep)[0]
        return [meta[i] for i in rows], d[rows]

    def decode_all(self, parts):
        """`decode` with every detection in its place: the records say which ones t3d_detect_nms kept (Decoded.keep; None without nms_iou)."""
        FLAGS = self.FLAGS
        meta = [m for p in parts for m in p['meta']]
        if not meta:
            return meta, None
        live = [p for p in parts if len(p['keep'])]
        ds = DeviceFrustumSet.from_device(self.rt, [p['out'] for p in live], [p['keep'] for p in live], [p['counts'] for p in live],
                                          [type2class[m[2]] for m in meta])
        source = DeviceEvalSource(self.ops['graph'], dataset=ds, seed=FLAGS.seed)
        res = SI.inference(self.sess, self.ops, None, None, self.B, prefix=FLAGS.pred_prefix, use_boxpc_fit_prob=FLAGS.use_boxpc_fit_prob,
                           source=source, n_batches=(ds.F + self.B - 1) // self.B, decode='device', want_seg=False,
                           nms=None if self.nms_iou is None else SI.NmsRequest(
                               self.nms_iou, self.nms_metric, self.nms_score, [m[1] for m in meta], [type2class[m[2]] for m in meta],
                               [m[4] for m in meta]))
        d = res.decoded[slice(0, ds.F)]
        if d.keep is not None and self.log:
            self.log('nms (%s IoU > %g, ranked by %s): kept %d of %d detections'
                     % (self.nms_metric, self.nms_iou, self.nms_score, int(d.keep.sum()), ds.F))
        return meta, d

    def detect(self, scenes, detections, scene_ids=None, batch_scenes=16):
        """scenes: [{'points' (n, C) fp64 upright depth, 'Rtilt', 'K'}] (FrustumExtractor.run); detections[s]: [(class name, box2d
        (xmin, ymin, xmax, ymax), prob)] of scene s.  -> per scene, a list of {'class', 'box2d', 'prob', 'score', 'label' (7,) = (h, w, l,
        tx, ty, tz, ry), 'corners' (8, 3)} in detection order; a detection whose frustum holds fewer than 5 points, or whose class is
        not whitelisted (or not among FLAGS.SUNRGBD_SEMI_TEST_CLS), or which t3d_detect_nms suppressed, has no entry.  (With nms_iou,
        scenes that share a scene id share their groups: give distinct ids.)"""
        if len(scenes) != len(detections):
            raise ValueError('%d scenes, detections of %d' % (len(scenes), len(detections)))
        scene_ids = list(range(len(scenes))) if scene_ids is None else list(scene_ids)
        parts, first = [], []
        for lo in range(0, len(scenes), batch_scenes):
            hi = min(lo + batch_scenes, len(scenes))
            parts.append(self.extract(scenes[lo:hi], detections[lo:hi], scene_ids[lo:hi]))
            first.append(lo)
        meta, d = self.decode_all(parts)
        out = [[] for _ in scenes]
        i = 0
        for lo, p in zip(first, parts):
            for s, _, name, box2d, prob in p['meta']:
                if d.keep is None or d.keep[i]:
                    out[lo + s].append(self.record(name, box2d, prob, d, i))
                i += 1
        return out

    @staticmethod
    def record(name, box2d, prob, d, i):
        return {'class': name, 'box2d': box2d, 'prob': prob, 'score': float(d.score[i]), 'label': d.label[i], 'corners': d.corners[i]}

    def predictions(self, meta, d):
        """test_semisup's 14-list of a detection run (the entries it fills for --from_rgb_detection; the rotation angles stayed on the
        device, the label rows carry them) with the decoded records attached."""
        n = len(meta)
        if d is None:
            return SI.Predictions([None, None, [], [], [], [], [], [], [], [], [], [], [], None])
        p = SI.Predictions([None, None, [None] * n, list(d.center), list(d.heading_cls), list(d.heading_res), list(d.size_cls),
                            list(d.size_res), [None] * n, [m[4] for m in meta],
                            [type2class[m[2]] for m in meta], [m[1] for m in meta], [m[3] for m in meta], None])
        p.decoded = d
        return p


def parser():
    p = argparse.ArgumentParser(description='3-D detections from SUN-RGBD scenes and 2-D detections, on the device', allow_abbrev=False)
    p.add_argument('--dataset_dir', default='mysunrgbd', help='SUN-RGBD root (<dir>/training/{image,calib,depth,label_dimension})')
    p.add_argument('--idx_path', required=True, help='index file of the images to run, e.g. mysunrgbd/training/val_data_idx.txt')
    p.add_argument('--rgb_detection_path', required=True, help='folder of 2-D detection files (sunrgbd_data --rgb_detection_path)')
    p.add_argument('--type_whitelist', nargs='+', default=list(SD.TYPE_WHITELIST), help='classes of detections to take')
    p.add_argument('--official_eval', action='store_true', help='print the lines of script_3Deval.m for the detections (evaluate_sunrgbd)')
    p.add_argument('--test_on', default='AB', choices=['A', 'B', 'AB'], help='set of classes --official_eval scores')
    NMS.add_arguments(p)
    return p


def main(argv=None, rt=None, log=print):
    """Every flag this parser does not know is test_semisup's (--seed serves the extraction and the network alike)."""
    args, rest = parser().parse_known_args(argv)
    FLAGS = TS.build_flags(list(rest))
    try:
        NMS.check_options(args.nms_iou, args.nms_metric, args.nms_score)
    except ValueError as e:
        parser().error(str(e))
    det = Detector(FLAGS, rt=rt, type_whitelist=args.type_whitelist, nms_iou=args.nms_iou, nms_metric=args.nms_metric,
                   nms_score=args.nms_score, log=log)
    valid = set(int(line.rstrip()) for line in open(args.idx_path))
    det_id, det_type, det_box2d, det_prob = SD.read_det_folder(args.rgb_detection_path)
    per_scene = collections.OrderedDict()
    for d, idx in enumerate(det_id):
        per_scene.setdefault(idx, []).append((det_type[d], det_box2d[d], det_prob[d]))
    ids = [i for i in per_scene if i in valid]
    dataset = SD.sunrgbd_object(args.dataset_dir, 'training')
    load = lambda idx: (dataset.get_calibration(idx), dataset.get_depth(idx))
    parts = []
    for batch in SD._scenes_in_batches(load, ids, 16, 8):
        scenes = [{'points': depth, 'Rtilt': calib.Rtilt, 'K': calib.K} for _, (calib, depth) in batch]
        parts.append(det.extract(scenes, [per_scene[idx] for idx, _ in batch], [idx for idx, _ in batch]))
    meta, d = det.decode(parts)
    predictions = det.predictions(meta, d)
    names = [m[2] for m in meta]
    log('%d detections of %d images' % (len(meta), len(ids)))
    if FLAGS.result_dir:
        SI.write_detection_results(FLAGS.result_dir, det.classes or sorted(set(names)), predictions, names)
        log('detection results written to %s' % FLAGS.result_dir)
    if args.official_eval:
        from transferable3d_amd import evaluate_sunrgbd as ES
        held = ES.official_predictions(sorted(set(ES.CLASS_NAMES[args.test_on]) | set(names)), predictions, names)
        ES.evaluate(None, args.dataset_dir, args.idx_path, args.test_on, rt=det.rt, log=log, predictions=held)
    return predictions


if __name__ == '__main__':
    main()
