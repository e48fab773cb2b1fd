#!/usr/bin/env python3
"""Time of t3d_scene_range and t3d_detect_visibility (csrc/range.hip).  Load: the 16 generated scenes of 730 x 530 pixels at stride 1 that
tools/bench_scene_synth.py casts (about 380 000 points each, six columns), left on the device as the extraction leaves them, and boxes
generated in front of, around and behind what their range maps show.

Three steps, each a child process under a time limit of its own (`timeout -k 10`), run in this order; a step that fails ends the run:
  compare   one scene through the device and through the NumPy specification (tests/fake_visibility.py): the range map and its counts
            equal as bytes; then one batch of boxes against that map with K = 9 candidates in mode 1: profile, measures, choice, flags
            and the output boxes equal as bytes;
  range     after a warm-up pass, `--passes` passes of t3d_scene_range over the 16 scenes, timed with device events around the call
            alone (inputs uploaded and outputs allocated outside): the median, next to the bytes it reads -- points x ld x 8, counting
            whole rows, since a row's unused columns share cache lines with the used ones -- and the cells it fills;
  detect    the same for t3d_detect_visibility on `--boxes` boxes in the 16 scenes, with K = 1 (what `detect --visibility` launches) and
            with K = 9 in mode 1, next to the bytes read: 31 floats and an index per box, plus one cell of the map per ray cast
            (cells_visited x 4; the calibration rows stay in cache).
Writes profiles/visibility_bench.json (`--out`) and prints it as one JSON line.  A report, not a gate: it sets no pass mark.  Runs from a
source checkout only: the specification is the test suite's.

  python tools/bench_visibility.py [--scenes 16] [--passes 5] [--boxes 4096]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
LIMITS = {'compare': 300, 'range': 240, 'detect': 240}           # seconds per step
CELL, MARGIN, MIN_CHORD, MIN_GAIN = 4, 0.05, 0.1, 4
OFFSETS = {1: np.zeros(1), 9: (np.arange(9) - 4) * 0.025}


def boxes(lay, n, seed):
    """n boxes over the scenes `lay`: the label boxes of their objects, each slid along its viewing ray by up to 15 % and resized by up to
    20 % -> (label [n, 7], corners [n, 8, 3] fp32, scene index [n] int32)."""
    from transferable3d_amd import sunrgbd_data as SD, synth_scenes as SS
    r = np.random.RandomState(seed)
    W, H = lay[0]['W'], lay[0]['H']
    pool = [(s, SD.compute_box_3d(SD.SUNObject3d(SS.label_line(obj, sc['Rtilt'], sc['K'], W, H)))) for s, sc in enumerate(lay) for obj in sc['objects']]
    label, corners, index = np.zeros((n, 7), np.float32), np.zeros((n, 8, 3), np.float32), np.zeros(n, np.int32)
    for i in range(n):
        s, k = pool[r.randint(len(pool))]
        c = k.mean(0)
        k = c + (k - c) * r.uniform(0.8, 1.2)
        k = k + r.uniform(-0.15, 0.15) * np.array([c[0], 0.0, c[2]])
        corners[i], index[i] = k, s
        c = k.mean(0)
        label[i] = (k[:, 1].max() - k[:, 1].min(), 1.0, 1.0, c[0], k[:, 1].max(), c[2], 0.0)
    return label, corners, index


def scene_calib(lay):
    from transferable3d_amd.consistency import calib_row
    return np.stack([calib_row(sc['Rtilt'], sc['K'], (sc['W'], sc['H'])) for sc in lay])


def cast(rt, a):
    import bench_scene_floor as BF
    points, offsets, lay = BF.cast(rt, a)
    for sc in lay:
        sc['W'], sc['H'] = a.width, a.height
    return points, offsets, lay


def range_call(rt, points, offsets, lay):
    """The operands of one t3d_scene_range call on the device -> (args, kept-alive tensors, range, counts, dims, goff)."""
    import torch
    import fake_visibility as FV
    from transferable3d_amd import abi
    dev, S = rt.device, len(lay)
    dims, goff = FV.grids([(sc['W'], sc['H']) for sc in lay], CELL)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t = dict(off=up(offsets.astype(np.int64)), cal=up(scene_calib(lay)), index=up(np.arange(S, dtype=np.int32)), dims=up(dims), goff=up(goff))
    rng, counts = torch.zeros(int(goff[-1]), dtype=torch.int32, device=dev), torch.zeros(S, 4, dtype=torch.int32, device=dev)
    args = abi.SceneRangeArgs(S, int(points.stride(0)), CELL, S, abi.dptr(points), C.cast(C.c_void_p(t['off'].data_ptr()), abi.L), abi.dptr(t['cal']),
                              abi.iptr(t['index']), abi.iptr(t['dims']), C.cast(C.c_void_p(t['goff'].data_ptr()), abi.L), int(goff[-1]), 0,
                              C.cast(C.c_void_p(rng.data_ptr()), abi.U32), abi.iptr(counts))
    return args, t, rng, counts, dims, goff


def detect_call(rt, label, corners, index, t, rng, K, mode):
    import torch
    from transferable3d_amd import abi
    dev, n, S = rt.device, len(label), int(t['dims'].shape[0])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d = dict(label=up(label), corners=up(corners.reshape(n, 24)), index=up(index), profile=torch.zeros(n * K, 6, dtype=torch.int32, device=dev),
             measures=torch.zeros(n, 3, dtype=torch.float64, device=dev), choice=torch.zeros(n, dtype=torch.int32, device=dev),
             flags=torch.zeros(n, dtype=torch.int32, device=dev), label_out=torch.zeros(n, 7, device=dev), corners_out=torch.zeros(n, 24, device=dev))
    o = (C.c_double * abi.VIS_MAX_OFFSETS)(*[float(v) for v in OFFSETS[K]])
    args = abi.DetectVisibilityArgs(n, S, mode, K, CELL, MIN_GAIN, 0, abi.fptr(d['label']), abi.fptr(d['corners']), abi.iptr(d['index']), abi.dptr(t['cal']),
                                    abi.iptr(t['dims']), C.cast(C.c_void_p(t['goff'].data_ptr()), abi.L), C.cast(C.c_void_p(rng.data_ptr()), abi.U32),
                                    int(rng.numel()), MARGIN, MIN_CHORD, o, abi.iptr(d['profile']), abi.dptr(d['measures']), abi.iptr(d['choice']),
                                    abi.iptr(d['flags']), abi.fptr(d['label_out']), abi.fptr(d['corners_out']))
    return args, d


def step(a):
    import torch
    import bench_scene_floor as BF
    import fake_visibility as FV
    from transferable3d_amd import abi
    from transferable3d_amd.engine import Runtime
    if not torch.cuda.is_available():
        raise SystemExit('bench_visibility.py times launches on the device: no GPU found')
    rt = Runtime()
    one = a.step == 'compare'
    points, offsets, lay = cast(rt, argparse.Namespace(**dict(vars(a), scenes=1)) if one else a)
    args, t, rng, counts, dims, goff = range_call(rt, points, offsets, lay)
    call = lambda: abi.check(rt.lib.t3d_scene_range(C.byref(args), rt.stream()), 't3d_scene_range')
    rec = {}
    if a.step == 'compare':
        call()
        p = points.cpu().numpy()
        want = FV.scene_range_batch(p, offsets, scene_calib(lay), [0], dims, goff, int(goff[-1]), CELL)
        got = rng.cpu().numpy().view(np.uint32), counts.cpu().numpy()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), 'the range map differs from the specification'
        label, corners, index = boxes(lay, 256, a.seed)
        dargs, d = detect_call(rt, label, corners, index, t, rng, 9, 1)
        abi.check(rt.lib.t3d_detect_visibility(C.byref(dargs), rt.stream()), 't3d_detect_visibility')
        spec = FV.detect_visibility(label, corners, index, scene_calib(lay), dims, goff, got[0], CELL, OFFSETS[9], MARGIN, MIN_CHORD, MIN_GAIN, 1)
        for name, w in zip(('profile', 'measures', 'choice', 'flags', 'label_out', 'corners_out'), spec):
            assert d[name].cpu().numpy().tobytes() == w.tobytes(), '%s differs from the specification' % name
        rec.update(compared_points=len(p), cells=int(goff[-1]), cells_filled=int(got[1][0, 2]), points_binned=int(got[1][0, 1]), compared_boxes=len(label),
                   boxes_moved=int(((spec[3] & abi.VIS_SNAPPED) != 0).sum()), rays_of_the_boxes=int(spec[0][:, 4, 0].sum()))
    elif a.step == 'range':
        rec = BF.timed(rt, call, a.passes)
        n, ld, c = int(points.shape[0]), int(points.shape[1]), counts.cpu().numpy()
        rec.update(scenes=len(lay), points=n, ld=ld, cell=CELL, cells=int(goff[-1]), bytes_read=n * ld * 8, bytes_of_the_maps=int(goff[-1]) * 4,
                   gb_per_s=round(n * ld * 8 / (rec['ms_median'] * 1e-3) / 1e9, 1), ms_per_scene=round(rec['ms_median'] / len(lay), 4),
                   points_binned=int(c[:, 1].sum()), cells_filled=int(c[:, 2].sum()))
    else:
        call()
        label, corners, index = boxes(lay, a.boxes, a.seed)
        for K, mode in ((1, 0), (9, 1)):
            dargs, d = detect_call(rt, label, corners, index, t, rng, K, mode)
            r = BF.timed(rt, lambda: abi.check(rt.lib.t3d_detect_visibility(C.byref(dargs), rt.stream()), 't3d_detect_visibility'), a.passes)
            prof = d['profile'].cpu().numpy().reshape(len(label), K, 6)
            rays = int(prof[:, :, 0].sum() + prof[:, :, 5].sum())
            r.update(boxes=len(label), K=K, mode=mode, rays_that_hit=rays, bytes_read_boxes=len(label) * (31 * 4 + 4), bytes_read_cells_of_hits=rays * 4,
                     us_per_box=round(1e3 * r['ms_median'] / len(label), 4), boxes_moved=int(((d['flags'] & abi.VIS_SNAPPED) != 0).sum().item()))
            rec['K%d' % K] = r
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=16)
    ap.add_argument('--width', type=int, default=730)
    ap.add_argument('--height', type=int, default=530)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--boxes', type=int, default=4096)
    ap.add_argument('--seed', type=int, default=2026)
    ap.add_argument('--step', choices=sorted(LIMITS), default=None, help='(internal) run one step in this process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'visibility_bench.json'))
    a = ap.parse_args()
    if a.step is not None:
        return step(a)
    rec = {'scenes': a.scenes, 'width': a.width, 'height': a.height, 'passes': a.passes}
    own = [x for k, v in vars(a).items() if k not in ('step', 'out') for x in ('--' + k, str(v))]
    for name in ('compare', 'range', 'detect'):
        cmd = ['timeout', '-k', '10', str(LIMITS[name]), sys.executable, os.path.abspath(__file__), '--step', name] + own
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit('step %s ended with status %d: nothing further is run' % (name, r.returncode))
        rec[{'compare': 'compare', 'range': 't3d_scene_range', 'detect': 't3d_detect_visibility'}[name]] = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
