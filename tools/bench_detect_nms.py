"""Time of t3d_detect_nms on a validation-set-sized synthetic load next to the host loop it spares the user: about 5000 images x 10
classes, group sizes drawn from 1..40, every group made of objects with jittered duplicates (what a 2-D detector hands over).

Three times, the device ones between events on the stream, median of `--reps` after a warm-up:
  nms_launches_ms      the three launches of t3d_detect_nms alone (lists, corners and scores already on the device);
  keep_copy_back_ms    the copy of `keep` ([n] uint8) to the host;
  host_loop_ms         the greedy loop in Python over the same boxes with the NumPy specification's IoU (tests/fake_nms.py), the corners
                       being on the host already.  It takes about half a millisecond per pair, so it is run over the first
                       `--host_groups` groups and scaled by the number of pairs that can touch (host_loop_ms_scaled); both are written.
The device answer for the sampled groups is compared with the host loop's (agree: how many boxes got the same keep bit -- the load is
random, pairs within rounding of the threshold are possible).

  python tools/bench_detect_nms.py --out profiles/detect_nms_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from transferable3d_amd import nms as NMS                     # noqa: E402
from transferable3d_amd.engine import Runtime                 # noqa: E402


def boxes_to_corners(b):
    """[n, 7] (cx, cy, cz, l, w, h, ry) -> [n, 8, 3] fp32 in get_3d_box order."""
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1]) * b[:, 3:4] / 2
    sy = np.array([1, 1, 1, 1, -1, -1, -1, -1]) * b[:, 5:6] / 2
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1]) * b[:, 4:5] / 2
    c, s = np.cos(b[:, 6:7]), np.sin(b[:, 6:7])
    return np.stack([c * sx + s * sz + b[:, 0:1], sy + b[:, 1:2], -s * sx + c * sz + b[:, 2:3]], 2).astype(np.float32)


def synthetic(images, classes, max_group, seed):
    """-> (corners, score, image id, class id) with the boxes in random order (so that a group's members are scattered)."""
    r = np.random.RandomState(seed)
    sizes = r.randint(1, max_group + 1, images * classes)
    n = int(sizes.sum())
    group = np.repeat(np.arange(len(sizes)), sizes)
    # an object per ~3 boxes of a group; every box is a jittered copy of one of its group's objects
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    n_obj = np.maximum(1, sizes // 3)
    obj_of = first[group] // 3 + r.randint(0, 1 << 30, n) % n_obj[group]           # an object id, unique per group
    n_objs = int(obj_of.max()) + 1
    obj = np.concatenate([r.uniform([-3, -0.5, 1], [3, 0.5, 6], (n_objs, 3)), r.uniform(0.4, 2.0, (n_objs, 3)), r.uniform(-np.pi, np.pi, (n_objs, 1))], 1)
    b = obj[obj_of]
    b[:, 0:3] += r.normal(0, 0.12, (n, 3))
    b[:, 3:6] *= r.uniform(0.85, 1.15, (n, 3))
    b[:, 6] += r.normal(0, 0.15, n)
    order = r.permutation(n)
    return boxes_to_corners(b)[order], r.uniform(0, 1, n).astype(np.float32)[order], (group // classes)[order], (group % classes)[order]


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), [round(v, 4) for v in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--max_group', type=int, default=40)
    ap.add_argument('--threshold', type=float, default=0.25)
    ap.add_argument('--metric', default='3d', choices=NMS.METRICS)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_groups', type=int, default=150, help='groups the host loop is run over')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import fake_nms as FN
    rt = Runtime()
    corners, score, img, cls = synthetic(a.images, a.classes, a.max_group, a.seed)
    n = len(score)
    t0 = time.perf_counter()
    offsets, members = NMS.groups_of(img, cls)
    groups_ms = (time.perf_counter() - t0) * 1e3
    dev = NMS.DeviceNms(rt)
    d_corners, d_score = torch.from_numpy(corners.reshape(n, 24)).to(rt.device), torch.from_numpy(score).to(rt.device)
    keep, _, _ = dev.run(d_corners, d_score, offsets, members, a.threshold, a.metric)
    torch.cuda.synchronize()
    launch_ms, launch_all = event_ms(dev.relaunch, a.reps)
    copy_ms, copy_all = event_ms(lambda: keep.cpu(), a.reps)
    got = keep.cpu().numpy()
    # the host loop over the first groups
    G = min(a.host_groups, len(offsets) - 1)
    k64 = corners.astype(np.float64)
    t0 = time.perf_counter()
    cache = {}
    want, _, _ = FN.greedy_nms(k64, score, offsets[:G + 1], members, a.threshold, FN.IOU2D if a.metric == 'bev' else FN.IOU3D, cache=cache)
    host_ms = (time.perf_counter() - t0) * 1e3
    sampled = members[:offsets[G]]
    agree = int((got[sampled] == want[sampled]).sum())
    # pairs that can touch, all groups: what the host loop's time is proportional to
    centre, half = k64.mean(1), 0.5 * np.linalg.norm(k64[:, 0] - k64[:, 6], axis=1)
    pairs = 0
    for g in range(len(offsets) - 1):
        m = members[offsets[g]:offsets[g + 1]]
        d = np.linalg.norm(centre[m][:, None] - centre[m][None], axis=2) <= half[m][:, None] + half[m][None]
        pairs += (int(d.sum()) - len(m)) // 2
    out = dict(images=a.images, classes=a.classes, groups=int(len(offsets) - 1), boxes=n, largest_group=int(np.diff(offsets).max()),
               threshold=a.threshold, metric=a.metric, kept=int(got.sum()), reps=a.reps,
               nms_launches_ms=round(launch_ms, 4), keep_copy_back_ms=round(copy_ms, 4), groups_of_host_ms=round(groups_ms, 2),
               host_loop_groups=G, host_loop_boxes=int(len(sampled)), host_loop_pairs=len(cache), host_loop_ms=round(host_ms, 1),
               pairs_that_can_touch=pairs, host_loop_ms_scaled=round(host_ms * pairs / max(len(cache), 1), 0),
               host_loop_agrees_on=[agree, int(len(sampled))], nms_launches_ms_all=launch_all, keep_copy_back_ms_all=copy_all)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
