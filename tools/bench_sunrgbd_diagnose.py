#!/usr/bin/env python3
"""Time of the launches of t3d_sunrgbd_diagnose next to those of t3d_sunrgbd_eval on the same generated class at the real scale
(tests/sunrgbd_diagnose_check.generate: 5 000 images, 20 000 boxes, 50 000 detections over ten classes; one class of it, about 5 000
detections, 2 000 own boxes and 18 000 boxes of the other classes).  The inputs are packed and uploaded once per entry point; only
the launches are timed, with device events on the runtime's stream, the two alternating in one process, median and minimum of
`--reps` after `--warmup` of each.  Writes profiles/sunrgbd_diagnose_bench.json (`--out`) and prints it as one JSON line.  Not a gate:
no target is fixed; both times and their ratio are recorded.
Runs from a source checkout only: the generator is the test suite's (tests/sunrgbd_diagnose_check.py).

  python tools/bench_sunrgbd_diagnose.py [--cls 3] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import sunrgbd_diagnose_check as DK                               # noqa: E402
from transferable3d_amd import evaluate_sunrgbd as ES             # noqa: E402
from transferable3d_amd.engine import Runtime                     # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--cls', type=int, default=3, help='the class of the generated set to time')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=2026)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sunrgbd_diagnose_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sunrgbd_diagnose.py times launches on the device: no GPU found')
    rt = Runtime()
    det, gt, other = DK.generate(seed=a.seed, n_images=5000, n_gt=20000, n_det=50000)[a.cls]
    launch_eval, fetch_eval = ES._eval_prepare(det, gt, None, DK.T_F, rt)
    launch_diag, fetch_diag = ES._eval_prepare(det, gt, None, DK.T_F, rt, other=other, bg_threshold=DK.T_B)
    stream = torch.cuda.current_stream()
    times = {'eval': [], 'diagnose': []}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3
    for k in range(a.warmup + a.reps):
        for name, fn in (('eval', launch_eval), ('diagnose', launch_diag)):         # alternating: both see the same machine
            us = timed(fn)
            if k >= a.warmup:
                times[name].append(us)
    e, d = fetch_eval(), fetch_diag()
    assert all(e[k].tobytes() == d[k].tobytes() for k in e), 'the diagnosis changed an output of the evaluation'
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {'class': a.cls, 'detections': len(det['confidence']), 'boxes': len(gt['image']), 'other_boxes': len(other['image']),
           'reps': a.reps, 'warmup': a.warmup,
           'eval_launches_us_median': round(med['eval'], 1), 'eval_launches_us_min': round(float(np.min(times['eval'])), 1),
           'diagnose_launches_us_median': round(med['diagnose'], 1), 'diagnose_launches_us_min': round(float(np.min(times['diagnose'])), 1),
           'ratio_diagnose_over_eval': round(med['diagnose'] / med['eval'], 3),
           'ap': float(d['ap'][0]), 'counts': dict(zip(ES.abi.DIAG_KINDS, [int(v) for v in d['counts']])),
           'gt_counts': dict(zip(ES.GT_STATES, [int(v) for v in d['gt_counts']])),
           'ap_fixed': dict(zip(ES.abi.DIAG_FIXES, [float(v) for v in d['ap_fixed']]))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
