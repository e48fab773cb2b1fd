#!/usr/bin/env python3
"""Wall time per batch of semisup_infer.inference with decode='host' (logits and six head tensors fetched, fp64 NumPy post-processing)
next to decode='device' (t3d_detect_decode behind the graph, one copy of the records at the end) on the SEMI_MODEL F inference graph at
B = 32, N = 2048, refine 1, synthetic frustums resident on the device.  Same process, same graph, one warm-up pass each, the two
alternated `--repeats` times; each pass ends in a device synchronise.  Prints one JSON line (profiles/detect_decode_bench.json).  Not a
gate.  The host pass also copies every batch's [B, N] labels back (DeviceEvalSource.load), the device pass does not: the difference is
the decode and that copy together."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from transferable3d_amd import semisup_infer as SI, test_semisup as TS    # noqa: E402
from transferable3d_amd.dataset import DeviceEvalSource, DeviceFrustumSet   # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    B, N = 32, 2048
    FLAGS = TS.build_flags(['--semi_type', 'F', '--use_one_hot', '--num_point', str(N), '--batch_size', str(B), '--refine', '1',
                            '--pred_prefix', 'F2_'])
    sess, ops = TS.get_model(FLAGS, B, N, FLAGS.NUM_CHANNELS)
    g = ops['graph']
    source = DeviceEvalSource(g, dataset=DeviceFrustumSet.synthetic(g.rt, a.batches * B, num_channel=6, seed=1), seed=1)

    def run(decode):
        t = time.perf_counter()
        SI.inference(sess, ops, None, None, B, prefix='F2_', source=source, n_batches=a.batches, decode=decode, want_seg=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.batches * 1e3
    times = {'host': [], 'device': []}
    for k in times:
        run(k)
    for _ in range(a.repeats):
        for k in times:
            times[k].append(run(k))
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({'B': B, 'N': N, 'batches_per_pass': a.batches, 'repeats': a.repeats, 'refine': 1,
                      'host_decode_ms_per_batch': round(med(times['host']), 4), 'device_decode_ms_per_batch': round(med(times['device']), 4),
                      'host_decode_ms_all': [round(v, 4) for v in times['host']], 'device_decode_ms_all': [round(v, 4) for v in times['device']]}))


if __name__ == '__main__':
    main()
