#!/usr/bin/env python3
"""What test-time augmentation (t3d_detect_ensemble, detect --tta K) costs.

1. The two launches of t3d_detect_ensemble alone on `--boxes` (default a million) synthetic detections at V = 4 and V = 8 views: every
   detection an object with jittered copies as its views (tools/bench_detect_nms.py's jitter), the odd views stored mirrored, labels,
   weights and angles on the device already.  Between two events on the stream, median of `--reps` (5) passes after a warm-up.
2. The inference loop per batch without views and with the four views of --tta 4 --tta_flip (semisup_infer.inference(decode='device',
   views=...): assemble, network and decode once per view and batch, one ensemble call at the end) on the SEMI_MODEL F inference graph at
   B = 32, N = 2048, refine 1, synthetic frustums resident on the device -- the method of tools/bench_detect_consistency.py: same
   process, same graph, one warm-up pass each, the two alternated `--repeats` times, each pass ended by a device synchronise, the median.

The ensemble is compared with nothing that existed before it, and K views are expected to cost about K passes of the network: no target
was set.  Prints one JSON line and writes it to --out.

  python tools/bench_detect_ensemble.py --out profiles/detect_ensemble_bench.json
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
from transferable3d_amd import ensemble as EN, semisup_infer as SI, test_semisup as TS      # noqa: E402
from transferable3d_amd.dataset import DeviceEvalSource, DeviceFrustumSet                  # noqa: E402
from transferable3d_amd.engine import Runtime                                               # noqa: E402


def synthetic(n, V, seed=0):
    """(labels [V, n, 7], weights [V, n], rot [n]) fp32: objects as tools/bench_detect_nms.py draws them, a jittered copy per view."""
    r = np.random.RandomState(seed)
    obj = np.concatenate([r.uniform([-3, -0.5, 1], [3, 0.5, 6], (n, 3)), r.uniform(0.4, 2.0, (n, 3)), r.uniform(-np.pi, np.pi, (n, 1))], 1)
    labels = np.zeros((V, n, 7), np.float32)
    for v in range(V):
        c = obj.copy()
        c[:, 0:3] += r.normal(0, 0.12, (n, 3))
        c[:, 3:6] *= r.uniform(0.85, 1.15, (n, 3))
        c[:, 6] += r.normal(0, 0.15, n)
        labels[v] = np.stack([c[:, 5], c[:, 4], c[:, 3], c[:, 0], c[:, 1] + c[:, 5] / 2, c[:, 2], c[:, 6]], 1)
    rot = (np.pi / 2 + r.uniform(-0.6, 0.6, n)).astype(np.float32)
    for v in range(1, V, 2):                        # the odd views as a mirrored run decodes them
        a, tx, tz = rot.astype(np.float64), labels[v, :, 3].astype(np.float64), labels[v, :, 5].astype(np.float64)
        xc, zc = tx * np.cos(a) - tz * np.sin(a), tx * np.sin(a) + tz * np.cos(a)
        labels[v, :, 3], labels[v, :, 5] = -xc * np.cos(a) + zc * np.sin(a), xc * np.sin(a) + zc * np.cos(a)
        labels[v, :, 6] = np.pi - labels[v, :, 6] + 2 * a
    return labels, r.uniform(0.05, 1.0, (V, n)).astype(np.float32), rot


def corners_of(label):
    h, w, l, tx, ty, tz, ry = (label[:, k].astype(np.float64) for k in range(7))
    out = np.zeros((len(label), 8, 3))
    for c in range(8):
        x, y, z = (-l if c & 2 else l) / 2, (h if c < 4 else -h) / 2, (-w if (c + 1) & 2 else w) / 2
        out[:, c] = np.stack([np.cos(ry) * x + np.sin(ry) * z + tx, y + ty - h / 2, -np.sin(ry) * x + np.cos(ry) * z + tz], 1)
    return out.astype(np.float32)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(rt, n, V, reps, seed):
    labels, weights, rot = synthetic(n, V, seed)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(rt.device)
    dev = EN.DeviceEnsemble(rt)
    out = dev.run([up(labels[v]) for v in range(V)], [up(weights[v]) for v in range(V)], up(corners_of(labels[0]).reshape(n, 24)),
                  sum(1 << v for v in range(1, V, 2)), up(rot), 0.0, '3d')
    torch.cuda.synchronize()
    for _ in range(2):
        dev.relaunch()
    ms = [event_ms(dev.relaunch) for _ in range(reps)]
    agreement, votes = out[2].cpu().numpy(), out[5].cpu().numpy()
    return dict(views=V, boxes=n, pairs=n * V * (V - 1) // 2, launches_ms=round(float(np.median(ms)), 4), launches_ms_all=[round(t, 4) for t in ms],
                mean_agreement=round(float(agreement.mean()), 4), fused=int((votes > 0).sum()), votes=int(votes.sum()))


def loop(batches, repeats, K=4):
    B, N = 32, 2048
    FLAGS = TS.build_flags(['--semi_type', 'F', '--use_one_hot', '--num_point', str(N), '--batch_size', str(B), '--refine', '1', '--pred_prefix', 'F2_'])
    sess, ops = TS.get_model(FLAGS, B, N, FLAGS.NUM_CHANNELS)
    g = ops['graph']
    source = DeviceEvalSource(g, dataset=DeviceFrustumSet.synthetic(g.rt, batches * B, num_channel=6, seed=1), seed=1)
    req = EN.EnsembleRequest(EN.views_of(K, True, 1))

    def run(with_views):
        t = time.perf_counter()
        SI.inference(sess, ops, None, None, B, prefix='F2_', source=source, n_batches=batches, decode='device', want_seg=False,
                     views=req if with_views else None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / batches * 1e3
    times = {False: [], True: []}
    for k in times:
        run(k)
    for _ in range(repeats):
        for k in times:
            times[k].append(run(k))
    med = lambda v: sorted(v)[len(v) // 2]
    return {'B': B, 'N': N, 'batches_per_pass': batches, 'repeats': repeats, 'refine': 1, 'views': K,
            'loop_ms_per_batch': round(med(times[False]), 4), 'loop_with_views_ms_per_batch': round(med(times[True]), 4),
            'views_ratio': round(med(times[True]) / med(times[False]), 3),
            'loop_ms_all': [round(v, 4) for v in times[False]], 'loop_with_views_ms_all': [round(v, 4) for v in times[True]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--boxes', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batches', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rt = Runtime()
    out = dict(ensemble_launches=[launches(rt, a.boxes, V, a.reps, a.seed) for V in (4, 8)], inference_loop=loop(a.batches, a.repeats))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
