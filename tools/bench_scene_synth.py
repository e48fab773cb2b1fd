#!/usr/bin/env python3
"""Time of the three launches of t3d_scene_raycast on 16 generated scenes of 730 x 530 pixels at stride 1, about 20 objects each (the
layouts of transferable3d_amd/synth_scenes.py with --max_objects 24, the fullest rooms of the first ids), with the default noise and drop
rate.  First one scene is compared with the NumPy specification (tests/fake_scene.py): hit, image, scene_offsets, visible, vis_box and
point_pixel equal, the rows within the bound t3d.h derives; the specification's own time on that scene is recorded beside the device's.
Then only the launches are timed, with device events on the runtime's stream (inputs uploaded and outputs allocated outside the events):
after a warm-up pass, `--passes` passes; the record holds the median, the minimum and the maximum.  Writes
profiles/scene_synth_bench.json (`--out`) and prints it as one JSON line.  A report, not a gate: there is no earlier version to compare
with.  Runs from a source checkout only: the specification is the test suite's.

  python tools/bench_scene_synth.py [--scenes 16] [--passes 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import fake_scene as FS                                           # noqa: E402
from transferable3d_amd import synth_scenes as SS                 # noqa: E402
from transferable3d_amd.engine import Runtime                     # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=16)
    ap.add_argument('--width', type=int, default=730)
    ap.add_argument('--height', type=int, default=530)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--seed', type=int, default=2026)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_synth_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_scene_synth.py times launches on the device: no GPU found')
    rt = Runtime()
    W, H = a.width, a.height
    lay = sorted((SS.layout(a.seed, sid, W, H, 24, 0.02) for sid in range(1, 4 * a.scenes + 1)), key=lambda s: -s['n_objects'])[:a.scenes]
    o = SS.DEFAULTS
    kw = dict(stride=1, seed=a.seed, noise_a=o['noise_a'], p_drop=o['p_drop'], max_range=o['max_range'], min_cos2=o['min_cos'] ** 2)
    caster = SS.SceneCaster(rt, H, W, **kw)
    # the results first, on one scene
    got = caster.run(lay[:1])
    s = lay[0]
    t0 = time.perf_counter()
    hit, img, t, d, u, v = FS.cast_scene(s['Rtilt'].reshape(9), s['K'].reshape(9), s['room'], s['parts'], H, W, kw['max_range'], kw['min_cos2'])
    rows, pixel, (dd, tt, g) = FS.emit_scene(hit, img, t, d, u, v, W, 1, a.seed, s['id'], kw['noise_a'], kw['p_drop'])
    vis, box = FS.stats(hit, pixel, s['parts']['owner'], u, v, H, W)
    spec_s = time.perf_counter() - t0
    assert np.array_equal(got['hit'][0].reshape(-1), hit) and np.array_equal(got['image'][0].reshape(-1, 3), img)
    assert np.array_equal(got['point_pixel'], pixel) and got['scene_offsets'].tolist() == [0, len(rows)]
    assert np.array_equal(got['visible'][0], vis) and np.array_equal(got['vis_box'][0], box)
    bound = 2.0 ** -52 * (8.0 * np.abs(dd) * (kw['noise_a'] * tt * tt * np.abs(g))[:, None] + 3.0 * np.abs(rows[:, :3]))
    err = np.abs(got['points'][:, :3] - rows[:, :3])
    assert (err <= bound).all() and np.array_equal(got['points'][:, 3:], rows[:, 3:])
    caster.run(lay, timed=True, on_device=True)                    # the warm-up pass
    ms = []
    for _ in range(a.passes):
        out = caster.run(lay, timed=True, on_device=True)
        ms.append(caster.last_kernel_ms)
    n_points = int(out['scene_offsets'][-1].item())
    rec = {'scenes': len(lay), 'width': W, 'height': H, 'stride': 1, 'objects_per_scene': [s['n_objects'] for s in lay],
           'parts_per_scene': [len(s['parts']) for s in lay], 'points': n_points, 'passes': a.passes,
           'launches_ms_median': round(float(np.median(ms)), 3), 'launches_ms_min': round(min(ms), 3), 'launches_ms_max': round(max(ms), 3),
           'launches_ms_per_scene': round(float(np.median(ms)) / len(lay), 4),
           'rays_per_second': round(len(lay) * W * H / (float(np.median(ms)) * 1e-3)),
           'specification_one_scene_s': round(spec_s, 2), 'specification_scene_objects': lay[0]['n_objects'],
           'worst_row_error_over_bound': float(np.max(err / np.maximum(bound, 1e-300)))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
