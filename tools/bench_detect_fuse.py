"""What box voting (t3d_detect_fuse, detect --nms_fuse) adds to the NMS launches, on the validation-set-sized synthetic load of
tools/bench_detect_nms.py: about 5000 images x 10 classes, group sizes drawn from 1..40, every group made of objects with jittered
duplicates.  Lists, labels, corners and scores are on the device already.

Two times between events on the stream, in alternated passes (A, B, A, B, ...) after a warm-up, median of `--reps` each:
  nms_launches_ms        the three launches of t3d_detect_nms alone;
  nms_fuse_launches_ms   the same three launches followed by the two of t3d_detect_fuse.
fuse_added_ms is their difference and fuse_added_ratio that difference over nms_launches_ms: there is no fusion before this entry point,
so the NMS launches on the same card are the baseline.  No target was set in advance.

  python tools/bench_detect_fuse.py --out profiles/detect_fuse_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_detect_nms import synthetic                        # noqa: E402
from transferable3d_amd import nms as NMS                     # noqa: E402
from transferable3d_amd.engine import Runtime                 # noqa: E402


def labels_of(corners):
    """[n, 8, 3] in get_3d_box order -> [n, 7] fp32 (h, w, l, tx, ty, tz, ry), ty the bottom of the box."""
    k = corners.astype(np.float64)
    l, w, h = (np.linalg.norm(k[:, a] - k[:, b], axis=1) for a, b in ((1, 2), (0, 1), (0, 4)))
    c = k.mean(1)
    e = k[:, 0] - k[:, 3]                                     # the l edge: (cos ry, 0, -sin ry) * l
    return np.stack([h, w, l, c[:, 0], c[:, 1] + h / 2, c[:, 2], np.arctan2(-e[:, 2], e[:, 0])], 1).astype(np.float32)


def event_ms(fn):
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
    ap.add_argument('--vote_threshold', type=float, default=None, help='default: --threshold')
    ap.add_argument('--metric', default='3d', choices=NMS.METRICS)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rt = Runtime()
    corners, score, img, cls = synthetic(a.images, a.classes, a.max_group, a.seed)
    n = len(score)
    offsets, members = NMS.groups_of(img, cls)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(rt.device)
    d_corners, d_score, d_label = up(corners.reshape(n, 24)), up(score), up(labels_of(corners))
    nms, fuse = NMS.DeviceNms(rt), NMS.DeviceFuse(rt)
    keep, _, _ = nms.run(d_corners, d_score, offsets, members, a.threshold, a.metric)
    vote = a.threshold if a.vote_threshold is None else a.vote_threshold
    _, _, votes = fuse.run(nms, d_label, d_corners, d_score, vote)
    torch.cuda.synchronize()

    def both():
        nms.relaunch()
        fuse.relaunch()

    for _ in range(3):
        nms.relaunch()
        both()
    alone, with_fuse = [], []
    for _ in range(a.reps):
        alone.append(event_ms(nms.relaunch))
        with_fuse.append(event_ms(both))
    t_nms, t_both = float(np.median(alone)), float(np.median(with_fuse))
    v = votes.cpu().numpy()
    out = dict(images=a.images, classes=a.classes, groups=int(len(offsets) - 1), boxes=n, largest_group=int(np.diff(offsets).max()),
               threshold=a.threshold, vote_threshold=vote, metric=a.metric, kept=int(keep.sum().item()), fused=int((v > 0).sum()),
               votes=int(v[v > 0].sum()), reps=a.reps, nms_launches_ms=round(t_nms, 4), nms_fuse_launches_ms=round(t_both, 4),
               fuse_added_ms=round(t_both - t_nms, 4), fuse_added_ratio=round((t_both - t_nms) / t_nms, 4),
               nms_launches_ms_all=[round(t, 4) for t in alone], nms_fuse_launches_ms_all=[round(t, 4) for t in with_fuse])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
