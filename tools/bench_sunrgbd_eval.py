#!/usr/bin/env python3
"""Wall time of the official SUN-RGBD evaluation on the device (evaluate_sunrgbd.compute_pr_curve_3d, one t3d_sunrgbd_eval call per
class) next to eval_det.eval_det (the Frustum-PointNets protocol: device IoU launch per class, Python pair list and claim pass) on
the same generated boxes (tests/sunrgbd_eval_check.generate: 5 000 images, 20 000 boxes, 50 000 detections, ten classes).  Same
process, one warm-up call each, host parsing excluded for both.  Prints one JSON line.  Not a gate: the two protocols differ.  One timed call each: no run-to-run spread is taken.
Runs from a source checkout only: the generator is the test suite's (tests/sunrgbd_eval_check.py)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import sunrgbd_eval_check as K                                     # noqa: E402
from transferable3d_amd import eval_det as E                      # noqa: E402
from transferable3d_amd import evaluate_sunrgbd as ES             # noqa: E402
from transferable3d_amd.engine import Runtime                     # noqa: E402


def corners(b, i):
    """The box struct as eval_det's (8,3) camera-frame corners: centre (X, -Z, Y), size 2 * coeffs, heading ry."""
    ry = np.arctan2(b['basis'][i, 1, 0], b['basis'][i, 0, 0])
    X, Y, Z = b['centroid'][i]
    return E.get_3d_box(2.0 * b['coeffs'][i], ry, (X, -Z, Y))


def main():
    import torch
    rt = Runtime()
    data = K.generate()
    official = lambda: [ES.compute_pr_curve_3d('c%d' % c, det, gt, None, 0.25, rt)['apScore'] for c, (det, gt) in data.items()]
    pred_all, gt_all = {}, {}
    for c, (det, gt) in data.items():
        for i in range(len(det['confidence'])):
            pred_all.setdefault(int(det['image'][i]), []).append(('c%d' % c, corners(det, i), float(det['confidence'][i])))
        for i in range(len(gt['image'])):
            gt_all.setdefault(int(gt['image'][i]), []).append(('c%d' % c, corners(gt, i)))
    fpn = lambda: E.eval_det(pred_all, gt_all, 0.25, rt=rt)[2]
    out = {'images': 5000, 'ground_truth': sum(len(g['image']) for _, g in data.values()), 'detections': sum(len(d['confidence']) for d, _ in data.values())}
    for name, fn in (('official_device_s', official), ('eval_det_s', fpn)):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        ap = fn()
        torch.cuda.synchronize()
        out[name] = round(time.perf_counter() - t, 4)
        out[name.replace('_s', '_mean_ap')] = float(np.mean(list(ap.values()) if isinstance(ap, dict) else ap))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
