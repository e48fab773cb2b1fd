"""Time of t3d_label_subset (the lists and class groups of a data set, built where `cls` lies) next to the host path it replaces:
cls.cpu() + the NumPy construction of DeviceFrustumSet.class_groups + the upload of members / offsets.  Both are wall-clock times of
the whole call, synchronised, median of `--reps` after a warm-up; docs/EXPERIMENTS.md records the numbers.

  python tools/bench_label_subset.py --frustums 96 65536
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transferable3d_amd.dataset import DeviceFrustumSet      # noqa: E402
from transferable3d_amd.engine import Runtime                 # noqa: E402


def host_groups(ds, subset):
    """The host construction: DeviceFrustumSet.class_groups(subset) with its cls.cpu() round trip and the two uploads."""
    cls = ds.cls.cpu().numpy()
    idx = np.asarray(subset, np.int32)
    present = sorted(set(int(c) for c in cls[idx]))
    members = np.concatenate([idx[cls[idx] == c] for c in present]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([int((cls[idx] == c).sum()) for c in present])]).astype(np.int32)
    dev = ds.rt.device
    return torch.as_tensor(members).to(dev), torch.as_tensor(offsets).to(dev), len(present)


def median_us(fn, reps):
    for _ in range(5):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frustums', type=int, nargs='+', default=[96, 65536])
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    rt = Runtime()
    for F in a.frustums:
        r = np.random.RandomState(F)
        z = np.zeros
        ds = DeviceFrustumSet(rt, points=z((F, 6), np.float32), seg=z(F, np.int32), offsets=np.arange(F + 1), frustum_angle=z(F),
                              box_center=z((F, 3)), heading=z(F), size=np.ones((F, 3)), cls=r.randint(0, 10, size=F))
        member = (r.uniform(size=F) < 0.5).astype(np.uint8)
        subset = np.nonzero(member)[0]
        dev_us, dev_min = median_us(lambda: ds.label_subset(member=member), a.reps)
        host_us, host_min = median_us(lambda: host_groups(ds, subset), a.reps)
        print(json.dumps(dict(F=F, label_subset_us=round(dev_us, 1), label_subset_min_us=round(dev_min, 1), host_class_groups_us=round(host_us, 1),
                              host_class_groups_min_us=round(host_min, 1))))


if __name__ == '__main__':
    main()
