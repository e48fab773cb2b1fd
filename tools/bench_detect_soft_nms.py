"""Time of t3d_detect_soft_nms next to t3d_detect_nms on the load of tools/bench_detect_nms.py: about 5000 images x 10 classes, group
sizes drawn from 1..40 (a million boxes in 50 000 groups), every group made of objects with jittered duplicates.

The launches alone (lists, corners and scores already on the device; DeviceSoftNms.relaunch / DeviceNms.relaunch), between events on the
stream.  A pass times, one after the other in the same process, Soft-NMS gaussian, Soft-NMS linear at the hard suppression's threshold and
t3d_detect_nms at that threshold; the median of `--passes` passes after a warm-up pass is reported with every sample.  Before anything is
timed, the device answers for the first `--spec_groups` groups are compared with the NumPy specification (tests/fake_soft_nms.py): keep and
n_decays by count of equal boxes (the load is random, decisions within rounding are possible), score_out by the largest difference.
Soft-NMS does one IoU per live pair and step, the hard suppression one per pair above the diagonal, in three launches: the ratio is
reported, there is no pass bar.  One group of 1024 boxes (tests/nms_check.big_case) is timed as well: its selections are sequential.

  python tools/bench_detect_soft_nms.py --out profiles/detect_soft_nms_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from transferable3d_amd import nms as NMS                     # noqa: E402
from transferable3d_amd.engine import Runtime                 # noqa: E402
from bench_detect_nms import synthetic                        # noqa: E402


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--max_group', type=int, default=40)
    ap.add_argument('--threshold', type=float, default=0.25)
    ap.add_argument('--sigma', type=float, default=0.5)
    ap.add_argument('--min_score', type=float, default=0.001)
    ap.add_argument('--metric', default='3d', choices=NMS.METRICS)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--spec_groups', type=int, default=100, help='groups the specification is run over')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import fake_soft_nms as FS
    import nms_check as NC
    rt = Runtime()
    corners, score, img, cls = synthetic(a.images, a.classes, a.max_group, a.seed)
    n = len(score)
    offsets, members = NMS.groups_of(img, cls)
    d_corners, d_score = torch.from_numpy(corners.reshape(n, 24)).to(rt.device), torch.from_numpy(score).to(rt.device)
    soft = {m: NMS.DeviceSoftNms(rt) for m in NMS.SOFT_METHODS}
    hard = NMS.DeviceNms(rt)
    G = min(a.spec_groups, len(offsets) - 1)
    sampled = members[:offsets[G]]
    out = dict(images=a.images, classes=a.classes, groups=int(len(offsets) - 1), boxes=n, largest_group=int(np.diff(offsets).max()),
               threshold=a.threshold, sigma=a.sigma, min_score=a.min_score, metric=a.metric, passes=a.passes, spec_groups=G, spec_boxes=int(len(sampled)))
    metric_id = FS.IOU2D if a.metric == 'bev' else FS.IOU3D
    for m, dev in soft.items():
        got = [t.cpu().numpy() for t in dev.run(d_corners, d_score, offsets, members, m, a.threshold if m == 'linear' else None, a.sigma, a.min_score, a.metric)]
        want = FS.soft_nms(corners, score, offsets[:G + 1], members, m, a.threshold, a.sigma, a.min_score, metric_id)
        same = (got[1][sampled] == want.keep[sampled]) & (got[3][sampled] == want.n_decays[sampled])
        diff = np.abs(got[0][sampled].astype(np.float64) - want.score_out[sampled])[same]
        out[m] = dict(kept=int(got[1].sum()), decayed=int((got[3] > 0).sum()), spec_agrees_on=[int(same.sum()), int(len(sampled))],
                      largest_score_difference=float(diff.max(initial=0.0)))
        if same.sum() < 0.99 * len(sampled) or diff.max(initial=0.0) > 1e-3:
            raise SystemExit('the device answers differ from the specification: %r' % (out[m],))
    keep, _, _ = hard.run(d_corners, d_score, offsets, members, a.threshold, a.metric)
    out['hard_kept'] = int(keep.sum().item())
    torch.cuda.synchronize()
    runs = [('gaussian', soft['gaussian'].relaunch), ('linear', soft['linear'].relaunch), ('hard', hard.relaunch)]
    times = {k: [] for k, _ in runs}
    for p in range(a.passes + 1):                    # pass 0 warms up
        for k, fn in runs:
            t = once_ms(fn)
            if p:
                times[k].append(round(t, 4))
    for k, t in times.items():
        out[k + '_ms'], out[k + '_ms_all'] = float(np.median(t)), t
    out['gaussian_over_hard'] = round(out['gaussian_ms'] / out['hard_ms'], 3)
    out['linear_over_hard'] = round(out['linear_ms'] / out['hard_ms'], 3)
    # one group of 1024 boxes: 1024 sequential selections
    c = NC.big_case(a.metric, 0.25)
    k, s, off, mem = c.arrays()
    one = NMS.DeviceSoftNms(rt)
    one.run(torch.from_numpy(k.reshape(-1, 24)).to(rt.device), torch.from_numpy(s).to(rt.device), off, mem, 'gaussian', None, a.sigma, a.min_score, a.metric)
    one_hard = NMS.DeviceNms(rt)
    one_hard.run(torch.from_numpy(k.reshape(-1, 24)).to(rt.device), torch.from_numpy(s).to(rt.device), off, mem, 0.25, a.metric)
    torch.cuda.synchronize()
    t = {'group_1024_gaussian_ms': [], 'group_1024_hard_ms': []}
    for p in range(a.passes + 1):
        for key, fn in (('group_1024_gaussian_ms', one.relaunch), ('group_1024_hard_ms', one_hard.relaunch)):
            v = once_ms(fn)
            if p:
                t[key].append(round(v, 4))
    for key, v in t.items():
        out[key], out[key + '_all'] = float(np.median(v)), v
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
