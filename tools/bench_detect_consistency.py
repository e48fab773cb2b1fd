#!/usr/bin/env python3
"""Wall time per batch of semisup_infer.inference(decode='device') without and with a consistency request (t3d_detect_consistency behind
every batch's decode, one more small copy back at the end) on the SEMI_MODEL F inference graph at B = 32, N = 2048, refine 1, synthetic
frustums resident on the device: the method of tools/bench_detect_decode.py -- same process, same graph, one warm-up pass each, the two
alternated `--repeats` times, each pass ended by a device synchronise, the median reported.  The pass without a request runs the loop
as it was before the request existed (no launch, no buffer, no copy is added to it).

Beside it, the two launches alone on the buffers of the last batch: `--launches` back-to-back t3d_detect_decode launches and as many
t3d_detect_consistency launches between two events each.  Prints one JSON line (profiles/detect_consistency_bench.json).  Not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from transferable3d_amd import consistency as CS, semisup_infer as SI, test_semisup as TS    # noqa: E402
from transferable3d_amd.dataset import DeviceEvalSource, DeviceFrustumSet   # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    a = ap.parse_args()
    B, N = 32, 2048
    FLAGS = TS.build_flags(['--semi_type', 'F', '--use_one_hot', '--num_point', str(N), '--batch_size', str(B), '--refine', '1',
                            '--pred_prefix', 'F2_'])
    sess, ops = TS.get_model(FLAGS, B, N, FLAGS.NUM_CHANNELS)
    g = ops['graph']
    n = a.batches * B
    source = DeviceEvalSource(g, dataset=DeviceFrustumSet.synthetic(g.rt, n, num_channel=6, seed=1), seed=1)
    r = np.random.RandomState(2)
    x0, y0 = r.uniform(0, 400, n), r.uniform(0, 300, n)
    K = [[529.5, 0.0, 365.0], [0.0, 529.5, 265.0], [0.0, 0.0, 1.0]]
    req = CS.ConsistencyRequest(np.stack([x0, y0, x0 + r.uniform(30, 300, n), y0 + r.uniform(30, 200, n)], 1),
                                [CS.calib_row(np.eye(3), K, (730, 530))] * (n // 8), np.arange(n) // 8)

    def run(with_request):
        t = time.perf_counter()
        res = SI.inference(sess, ops, None, None, B, prefix='F2_', source=source, n_batches=a.batches, decode='device', want_seg=False,
                           consistency=req if with_request else None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.batches * 1e3, res
    times = {False: [], True: []}
    for k in times:
        run(k)
    for _ in range(a.repeats):
        for k in times:
            times[k].append(run(k)[0])
    med = lambda v: sorted(v)[len(v) // 2]

    # the two launches alone, on what the last batch left in the graph's buffers
    logits, box, s1, delta, fit = SI.decode_sources(ops, 'F2_', False)
    dec, con = SI.DeviceDecode(g.rt, B, N), CS.DeviceConsistency(g.rt, B, N, CS.ConsistencyRequest(req.box2d[:B], req.calib_rows, req.calib_index[:B]))
    xyz, rot = sess.g.inputs.pc, sess.g.inputs.rot_frust
    launch = {'decode': lambda: dec.launch(0, B, B, logits, box, s1, delta, fit, rot),
              'consistency': lambda: con.launch(0, B, B, xyz, int(xyz.stride(0)), logits, dec.sec['corners'], rot)}
    alone = {}
    for k, fn in launch.items():
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream()
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(a.launches):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        alone[k] = e0.elapsed_time(e1) / a.launches * 1e3
    print(json.dumps({'B': B, 'N': N, 'batches_per_pass': a.batches, 'repeats': a.repeats, 'refine': 1,
                      'loop_ms_per_batch': round(med(times[False]), 4), 'loop_with_consistency_ms_per_batch': round(med(times[True]), 4),
                      'loop_ms_all': [round(v, 4) for v in times[False]], 'loop_with_consistency_ms_all': [round(v, 4) for v in times[True]],
                      'decode_launch_us': round(alone['decode'], 2), 'consistency_launch_us': round(alone['consistency'], 2),
                      'launches': a.launches}))


if __name__ == '__main__':
    main()
