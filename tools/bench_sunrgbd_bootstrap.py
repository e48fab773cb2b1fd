#!/usr/bin/env python3
"""Wall time of the bootstrap over images on the device (t3d_bootstrap_weights once, then one t3d_sunrgbd_eval_bootstrap call per
class) on the generated boxes of tools/bench_sunrgbd_eval.py (tests/sunrgbd_eval_check.generate: ten classes, 5 050 image ids, 20 000
boxes, 50 000 detections) with R = 2 000 replicates.

The results are compared first: for --check replicates (default 3) every class's replicate is evaluated literally -- the resampled data
set built on the host (tests/fake_bootstrap.expand), scored by t3d_sunrgbd_eval -- and the counts must agree exactly, the AP within 1e-12.
Then the launches alone are timed (inputs uploaded before, nothing copied back; one synchronisation behind the ten classes): the median
of 5 passes after a warm-up, for the weights, for the ten bootstrap calls, and for the ten plain t3d_sunrgbd_eval calls they contain.
The comparison point is the naive route, R full evaluations: the launches of t3d_sunrgbd_eval on the literally expanded replicates,
timed on the --check replicates and SCALED to R (its host side -- building and uploading R data sets -- is left out, in its favour).
Prints one JSON line; --out FILE also writes it.  Runs from a source checkout only: generator and expansion are the test suite's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import fake_bootstrap as FB                                        # noqa: E402
import sunrgbd_eval_check as K                                     # noqa: E402
from transferable3d_amd import bootstrap as BS                    # noqa: E402
from transferable3d_amd import evaluate_sunrgbd as ES             # noqa: E402
from transferable3d_amd.engine import Runtime                     # noqa: E402


def median_s(fn, passes=5):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(passes):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return float(np.median(times)), times


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument('--replicates', type=int, default=2000)
    p.add_argument('--check', type=int, default=3, help='replicates that are also evaluated literally (compared, then timed and scaled)')
    p.add_argument('--out', default=None)
    args = p.parse_args()
    rt = Runtime()
    data = K.generate()
    idx_list = list(range(1 + max(int(max(d['image'].max(), g['image'].max())) for d, g in data.values())))
    R = args.replicates
    weights = BS.Weights(rt, len(idx_list), R, seed=0)
    t_weights, _ = median_s(lambda: BS.Weights(rt, len(idx_list), R, seed=0))
    w_host = weights.numpy()
    assert (w_host.sum(1) == len(idx_list)).all()
    cols = {c: (ES._columns(d['image'], idx_list, 'a detection'), ES._columns(g['image'], idx_list, 'a box')) for c, (d, g) in data.items()}
    boot = {c: ES._eval_prepare(d, g, None, 0.25, rt, boot=(weights,) + cols[c]) for c, (d, g) in data.items()}
    plain = {c: ES._eval_prepare(d, g, None, 0.25, rt) for c, (d, g) in data.items()}
    # the results first
    for launch, _ in boot.values():
        launch()
    got = {c: fetch()['boot'] for c, (_, fetch) in boot.items()}
    literal, worst = [], 0.0
    for r in range(args.check):
        for c, (d, g) in data.items():
            dd, gg = FB.expand(d, g, cols[c][0], cols[c][1], w_host[r])
            launch, fetch = ES._eval_prepare(dd, gg, None, 0.25, rt)
            launch()
            e = fetch()
            assert (got[c]['n_pos'][r], got[c]['n_tp'][r], got[c]['n_fp'][r]) == (len(gg['image']), int(e['is_tp'].sum()), int(e['is_fp'].sum())), (r, c)
            worst = max(worst, abs(got[c]['ap'][r] - e['ap'][0]))
            literal.append(launch)
    assert worst <= 1e-12, worst
    t_boot, boot_times = median_s(lambda: [launch() for launch, _ in boot.values()])
    t_plain, _ = median_s(lambda: [launch() for launch, _ in plain.values()])
    t_literal, _ = median_s(lambda: [launch() for launch in literal])
    mean_ap = np.mean(np.stack([got[c]['ap'] for c in data], 1), axis=1)
    out = {'classes': len(data), 'images': len(idx_list), 'ground_truth': sum(len(g['image']) for _, g in data.values()),
           'detections': sum(len(d['confidence']) for d, _ in data.values()), 'replicates': R, 'device': torch.cuda.get_device_name(0),
           'weights_s': round(t_weights, 6), 'bootstrap_launches_s': round(t_boot, 6), 'bootstrap_launches_passes_s': [round(t, 6) for t in boot_times],
           'of_which_plain_evaluation_s': round(t_plain, 6), 'curves_only_s': round(t_boot - t_plain, 6),
           'literal_checked_replicates': args.check, 'literal_checked_s': round(t_literal, 6),
           'literal_scaled_to_R_s': round(t_literal * R / max(args.check, 1), 4), 'literal_is_scaled': True,
           'worst_abs_ap_difference_on_checked': worst, 'mean_ap_summary': BS.summary({'mean': mean_ap}, 0.95)['mean_ap']}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
