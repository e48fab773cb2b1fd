#!/usr/bin/env python3
"""Time of the launches of t3d_sunrgbd_locparts next to those of t3d_sunrgbd_diagnose on the load of tools/bench_sunrgbd_diagnose.py
(tests/sunrgbd_diagnose_check.generate at the real scale: 5 000 images, 20 000 boxes, 50 000 detections over ten classes; one class of
it).  The inputs are packed and uploaded once per entry point.  First the results are compared: every output the two calls share must
have the same bytes.  Then only the launches are timed, with device events on the runtime's stream, the two alternating in one
process: after `--warmup` launches of each, `--passes` passes of `--reps` launches of each; a pass gives the median of its launches,
and the record holds the median, the minimum and the maximum of the passes.  Writes profiles/sunrgbd_locparts_bench.json (`--out`) and
prints it as one JSON line.  Not a gate: no target is fixed; both times, their difference and its spread are recorded.
Runs from a source checkout only: the generator is the test suite's (tests/sunrgbd_diagnose_check.py).

  python tools/bench_sunrgbd_locparts.py [--cls 3] [--passes 5] [--reps 10]
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
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10, help='launches of each entry point per pass')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=2026)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sunrgbd_locparts_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sunrgbd_locparts.py times launches on the device: no GPU found')
    rt = Runtime()
    det, gt, other = DK.generate(seed=a.seed, n_images=5000, n_gt=20000, n_det=50000)[a.cls]
    launch_diag, fetch_diag = ES._eval_prepare(det, gt, None, DK.T_F, rt, other=other, bg_threshold=DK.T_B)
    launch_parts, fetch_parts = ES._eval_prepare(det, gt, None, DK.T_F, rt, other=other, bg_threshold=DK.T_B, parts=True)
    launch_diag()
    launch_parts()
    d, p = fetch_diag(), fetch_parts()
    assert all(d[k].tobytes() == p[k].tobytes() for k in d), 'the split changed an output of the diagnosis'
    stream = torch.cuda.current_stream()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3
    for _ in range(a.warmup):
        timed(launch_diag)
        timed(launch_parts)
    passes = {'diagnose': [], 'locparts': []}
    for _ in range(a.passes):
        times = {'diagnose': [], 'locparts': []}
        for _ in range(a.reps):
            for name, fn in (('diagnose', launch_diag), ('locparts', launch_parts)):      # alternating: both see the same machine
                times[name].append(timed(fn))
        for name in passes:
            passes[name].append(float(np.median(times[name])))
    p2 = fetch_parts()
    assert all(p[k].tobytes() == p2[k].tobytes() for k in p), 'two runs differ'
    med = {k: float(np.median(v)) for k, v in passes.items()}
    added = [b - c for b, c in zip(passes['locparts'], passes['diagnose'])]
    kinds = p['kind']
    out = {'class': a.cls, 'detections': len(det['confidence']), 'boxes': len(gt['image']), 'other_boxes': len(other['image']),
           'matched_detections': int((p['gt_idx'] > 0).sum()), 'passes': a.passes, 'reps_per_pass': a.reps, 'warmup': a.warmup,
           'diagnose_launches_us_median': round(med['diagnose'], 1), 'diagnose_launches_us_passes': [round(v, 1) for v in passes['diagnose']],
           'locparts_launches_us_median': round(med['locparts'], 1), 'locparts_launches_us_passes': [round(v, 1) for v in passes['locparts']],
           'added_us_median': round(float(np.median(added)), 1), 'added_us_min': round(min(added), 1), 'added_us_max': round(max(added), 1),
           'ratio_locparts_over_diagnose': round(med['locparts'] / med['diagnose'], 3),
           'ap': float(p['ap'][0]), 'loc_detections': int((kinds == ES.abi.DIAG_KINDS.index('loc')).sum()),
           'ap_fixed_loc': float(p['ap_fixed'][ES.abi.DIAG_FIXES.index('loc')]),
           'ap_part': dict(zip(ES.abi.LOC_PARTS, [float(v) for v in p['ap_part']])),
           'part_counts': dict(zip(ES.abi.LOC_PARTS, [int(v) for v in p['part_counts']])),
           'part_boxes': dict(zip(ES.abi.LOC_PARTS, [int(v) for v in p['part_boxes']]))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
