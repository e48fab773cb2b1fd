#!/usr/bin/env python3
"""Time of the launches of t3d_rescore_features, t3d_rescore_fit and t3d_rescore_apply on a million generated detections with the seven
named features.  The stage buffers are generated and uploaded once; first the results are compared with the NumPy specification
(tests/fake_rescore.py): the non-transcendental feature columns bit for bit, the log columns within 2 ulps, the fitted coefficients
within the bound of tests/rescore_check.py, the applied confidences within 2^-50 relative.  Then only the launches are timed, with device
events on the runtime's stream: after a warm-up pass, `--passes` passes; the record holds the median, the minimum and the maximum of the
passes.  The fit is timed as enqueued -- all `max_iter` evaluations' launches, those behind the convergence returning at once -- and the
record says how many evaluations were accepted.  Writes profiles/rescore_bench.json (`--out`) and prints it as one JSON line.  A
report, not a gate: there is no earlier version to compare with.
Runs from a source checkout only: the specification is the test suite's.

  python tools/bench_rescore.py [--rows 1000000] [--passes 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import fake_rescore as FR                                         # noqa: E402
import rescore_check as RK                                        # noqa: E402
from transferable3d_amd import abi, rescore as RS                 # noqa: E402
from transferable3d_amd.engine import Runtime                     # noqa: E402


def generate(n, seed):
    """Stage buffers of n detections, a third of them on an object: those have the higher measures."""
    rng = np.random.RandomState(seed)
    on = rng.uniform(size=n) < 1.0 / 3.0
    mix = lambda lo, hi: np.clip(np.where(on, rng.normal(hi, 0.15, n), rng.normal(lo, 0.15, n)), 0.0, 1.0)
    prob = np.clip(np.where(on, rng.beta(5, 2, n), rng.beta(2, 2, n)), 0.0, 1.0).astype(np.float32)
    score = np.where(on, rng.normal(-1.0, 1.0, n), rng.normal(-2.0, 1.2, n)).astype(np.float32)
    reproj = np.zeros((n, 5))
    reproj[:, 4] = mix(0.3, 0.7)
    n_mask = rng.randint(5, 1200, n)
    n_both = (n_mask * mix(0.4, 0.8)).astype(np.int64)
    n_box = n_both + rng.randint(0, 400, n)
    counts = np.stack([n_mask, n_box, n_both, np.zeros(n, np.int64)], 1).astype(np.int32)
    view = mix(0.4, 0.75).astype(np.float32)
    flip = rng.uniform(size=n) < 0.1                              # label noise: the classes overlap
    return prob, score, reproj, counts, view, (on ^ flip).astype(np.uint8)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1000000)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--lam', type=float, default=1e-3)
    ap.add_argument('--seed', type=int, default=2026)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rescore_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rescore.py times launches on the device: no GPU found')
    rt = Runtime()
    n = a.rows
    prob, score, reproj, counts, view, y = generate(n, a.seed)
    dr = RS.DeviceRescore(rt, n, RS.FEATURES)
    bufs = [RK.dev(rt, v) for v in (prob, score, reproj, counts, view)]
    yd, rd = RK.dev(rt, y), RK.dev(rt, np.ones(n))
    launches = {'features': lambda: dr.features(*bufs), 'fit': lambda: dr.fit(yd, rd, a.lam), 'apply': lambda: dr.apply()}
    # the results first
    launches['features']()
    X = dr.X.cpu().numpy()
    want_X = FR.features(dr.mask, prob, score, reproj, counts, view)
    for k, name in enumerate(dr.names):
        if name in ('logit_prob', 'log_mask'):
            assert RK.ulps(X[:, k], want_X[:, k]).max() <= 2, name
        else:
            assert X[:, k].tobytes() == want_X[:, k].tobytes(), name
    launches['fit']()
    f = dr.fetch_fit()
    want = FR.fit(X, y, np.ones(n), a.lam)
    assert f['status'] == want['status'] == 0, (RS.status_names(f['status']), RS.status_names(want['status']))
    coef_diff = float(np.abs(f['coef_std'] - want['coef_std']).max())
    assert coef_diff <= RK.COEF_BOUND, coef_diff
    launches['apply']()
    out = dr.out.cpu().numpy()
    spec_out = FR.apply(f['coef'], X)
    apply_rel = float((np.abs(out - spec_out) / spec_out).max())
    assert apply_rel <= RK.APPLY_REL, apply_rel
    stream = torch.cuda.current_stream()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3
    for fn in launches.values():                                  # the warm-up pass
        timed(fn)
    passes = {k: [] for k in launches}
    for _ in range(a.passes):
        for k, fn in launches.items():
            passes[k].append(timed(fn))
    again = dr.fetch_fit()
    assert all(np.asarray(again[k]).tobytes() == np.asarray(f[k]).tobytes() for k in ('coef', 'coef_std', 'mean', 'scale', 'loss')), 'two runs differ'
    rec = {'rows': n, 'features': list(dr.names), 'lambda': a.lam, 'slices': abi.rescore_slices(n), 'passes': a.passes,
           'fit_evaluations_enqueued': 30, 'fit_evaluations_accepted': f['n_iter'], 'fit_loss_first': float(f['loss'][0]),
           'fit_loss_last': float(f['loss'][f['n_iter'] - 1]), 'n_pos': f['n_pos'],
           'coef_std_difference_to_specification': coef_diff, 'apply_relative_difference_to_specification': apply_rel}
    for k, v in passes.items():
        rec['%s_us_median' % k] = round(float(np.median(v)), 1)
        rec['%s_us_min' % k] = round(min(v), 1)
        rec['%s_us_max' % k] = round(max(v), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
