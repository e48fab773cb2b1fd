#!/usr/bin/env python3
"""The captured training step of stage b (Box-PC Fit net) and stage c (SEMI_MODEL F with the frozen Box-PC branch) with the Box-PC net's
representation A and B (--BOX_PC_MASK_REPRESENTATION), fp32 and bf16, at B = 32, N = 1024, C = 4: milliseconds per step from CUDA events
around `--steps` hipGraph replays after `--warmup`, one JSON line per (stage, representation, dtype).

  python tools/bench_boxpc_rep.py [--steps 50] [--warmup 10] [--only F:B:f32]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from transferable3d_amd.engine import Runtime  # noqa: E402
from transferable3d_amd.step import build_training_step, workload_flags  # noqa: E402
from transferable3d_amd.synthetic import make_batch  # noqa: E402


def time_step(workload, rep, dtype, steps, warmup, B=32, N=1024, C=4):
    flags = workload_flags(workload)
    flags.BOX_PC_MASK_REPRESENTATION = rep
    g, model, step, loss = build_training_step(Runtime(), workload, B, N, C, dtype=dtype, seed=1, c=flags, use_hip_graph=True)
    model.inputs.load(make_batch(B, N, C, seed=5, boxpc=(workload == 'boxpc')))
    for _ in range(max(warmup, 2)):                 # (the first run is eager, the second captures)
        step.run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step.run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return {'stage': 'b' if workload == 'boxpc' else 'c', 'representation': rep, 'dtype': dtype, 'B': B, 'N': N, 'C': C,
            'ms_per_step': round(ms, 4), 'frustums_per_s': round(B / ms * 1e3, 1), 'launches': step.n_launches(),
            'loss': float(loss), 'steps': steps, 'warmup': warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--only', default=None, help='workload:representation:dtype, e.g. F:B:f32 (one configuration, for a profiler)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cases = [(w, r, d) for w in ('boxpc', 'F') for r in ('A', 'B') for d in ('f32', 'bf16')]
    if a.only:
        cases = [tuple(a.only.split(':'))]
    for w, r, d in cases:
        print(json.dumps(time_step(w, r, d, a.steps, a.warmup)), flush=True)


if __name__ == '__main__':
    main()
