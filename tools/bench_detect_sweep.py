"""Time of the two sweep entry points next to the loop they replace, on the synthetic loads of tools/bench_detect_nms.py (about a million
boxes in 50 000 groups) and tests/sunrgbd_eval_check.generate (50 000 detections and 20 000 boxes over 10 classes), at M configurations
of K NMS thresholds (default 64 and 4).  A configuration lists a random 50 .. 100 % of the boxes and selects a random 50 .. 100 % of
the detections.

  sweep   one t3d_detect_nms_sweep call over the M configurations, then one t3d_sunrgbd_eval_sweep call per class;
  loop    the parent's way without its copies: M t3d_detect_nms calls on the restricted lists, then per class M t3d_sunrgbd_eval calls on
          the selected detections -- launches only, every list and box already on the device.

Same process, the four parts alternated (sweep NMS, loop NMS, sweep evaluation, loop evaluation) per pass, between events on the
stream, median of `--passes` after a warm-up pass; `spread` is max - min over the passes.  Before anything is timed the two ways are
compared on these very inputs: every keep row byte for byte and the counts exactly (asserted), the largest AP difference reported.

  python tools/bench_detect_sweep.py --out profiles/detect_sweep_bench.json
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
from transferable3d_amd import evaluate_sunrgbd as ES, nms as NMS      # noqa: E402
from transferable3d_amd.engine import Runtime                          # noqa: E402


def restricted(offsets, members, sel):
    """The lists without the boxes of sel == False (vectorised fake_sweep.restricted)."""
    take = sel[members]
    group = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    counts = np.bincount(group[take], minlength=len(offsets) - 1)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), members[take].astype(np.int32)


def timed(fn):
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
    ap.add_argument('--detections', type=int, default=50000)
    ap.add_argument('--M', type=int, default=64)
    ap.add_argument('--K', type=int, default=4)
    ap.add_argument('--metric', default='3d', choices=NMS.METRICS)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import bench_detect_nms as BN
    import sunrgbd_eval_check as SC
    rt = Runtime()
    r = np.random.RandomState(a.seed)
    M, K = a.M, a.K
    thresholds = [round(0.15 + 0.5 * k / max(K - 1, 1), 4) for k in range(K)]
    ct = np.asarray([m % K for m in range(M)], np.int32)

    # ---- the suppression
    corners, score, img, cls = BN.synthetic(a.images, a.classes, a.max_group, a.seed)
    n = len(score)
    offsets, members = NMS.groups_of(img, cls)
    listed = (r.uniform(size=(M, n)) < r.uniform(0.5, 1.0, (M, 1))).astype(np.uint8)
    d_corners, d_score = torch.from_numpy(corners.reshape(n, 24)).to(rt.device), torch.from_numpy(score).to(rt.device)
    sweep = NMS.DeviceNmsSweep(rt)
    keep, n_kept = sweep.run(d_corners, d_score, offsets, members, thresholds, ct, torch.from_numpy(listed).to(rt.device), a.metric)
    singles, same_rows = [], 0
    for m in range(M):
        dev = NMS.DeviceNms(rt)
        go, mem = restricted(offsets, members, listed[m] != 0)
        k1 = dev.run(d_corners, d_score, go, mem, thresholds[ct[m]], a.metric, fill=(0, -1, -1))[0]
        same_rows += int(torch.equal(k1, keep[m]))
        singles.append(dev)
    kept = n_kept.cpu().numpy()

    # ---- the evaluation
    data = SC.generate(seed=2026 + a.seed, n_det=a.detections)
    sweeps, loops, ev_masks = [], [], []
    for c, (det, gt) in sorted(data.items()):
        P = len(det['confidence'])
        mask = (r.uniform(size=(M, P)) < r.uniform(0.5, 1.0, (M, 1))).astype(np.uint8)
        mask[0] = 1
        sweeps.append(ES._eval_prepare(det, gt, None, 0.25, rt, sweep=(torch.from_numpy(mask).to(rt.device), None)))
        loops.append([ES._eval_prepare(ES.select_boxes(det, np.nonzero(mask[m])[0]), gt, None, 0.25, rt) for m in range(M)])
        ev_masks.append(mask)
    worst_ap, same_counts = 0.0, 0
    for (launch, fetch), per_m, mask in zip(sweeps, loops, ev_masks):
        launch()
        got = fetch()
        for m, (l1, f1) in enumerate(per_m):
            l1()
            ref = f1()
            worst_ap = max(worst_ap, abs(float(got['ap'][m]) - float(ref['ap'][0])))
            same_counts += int((got['n_det'][m], got['n_tp'][m], got['n_fp'][m]) == (int(mask[m].sum()), int(ref['is_tp'].sum()), int(ref['is_fp'].sum())))
    assert same_rows == M and same_counts == M * len(sweeps) and worst_ap <= 1e-9, (same_rows, same_counts, worst_ap)

    parts = {'nms_sweep': sweep.relaunch, 'nms_loop': lambda: [d.relaunch() for d in singles],
             'eval_sweep': lambda: [l() for l, _ in sweeps], 'eval_loop': lambda: [l() for per_m in loops for l, _ in per_m]}
    times = {k: [] for k in parts}
    for p in range(a.passes + 1):                       # (pass 0 warms up)
        for k, fn in parts.items():
            t = timed(fn)
            if p:
                times[k].append(t)
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: float(max(v) - min(v)) for k, v in times.items()}
    sweep_all = [x + y for x, y in zip(times['nms_sweep'], times['eval_sweep'])]
    loop_all = [x + y for x, y in zip(times['nms_loop'], times['eval_loop'])]
    out = dict(M=M, K=K, thresholds=thresholds, metric=a.metric, boxes=n, groups=int(len(offsets) - 1), largest_group=int(np.diff(offsets).max()),
               classes=len(sweeps), detections=int(sum(len(d['confidence']) for d, _ in data.values())),
               gt_boxes=int(sum(len(g['image']) for _, g in data.values())), passes=a.passes,
               kept_min_max=[int(kept.min()), int(kept.max())], keep_rows_equal=same_rows, eval_counts_equal=same_counts, worst_ap_difference=worst_ap,
               **{k + '_ms': round(v, 4) for k, v in med.items()}, **{k + '_spread_ms': round(v, 4) for k, v in spread.items()},
               sweep_ms=round(float(np.median(sweep_all)), 4), loop_ms=round(float(np.median(loop_all)), 4),
               sweep_spread_ms=round(max(sweep_all) - min(sweep_all), 4), loop_spread_ms=round(max(loop_all) - min(loop_all), 4),
               loop_over_sweep=round(float(np.median(loop_all)) / float(np.median(sweep_all)), 2),
               nms_loop_over_sweep=round(med['nms_loop'] / med['nms_sweep'], 2), eval_loop_over_sweep=round(med['eval_loop'] / med['eval_sweep'], 2),
               **{k + '_ms_all': [round(x, 4) for x in v] for k, v in times.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
