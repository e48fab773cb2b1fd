"""Time of t3d_render on a batch of scene-sized pictures next to the NumPy specification on the host: 16 views of 730 x 530 (the size of
a SUN-RGBD Kinect v2 image), 50 000 points and 20 boxes each, an image background under every view.

Times, the device ones between events on the stream, median of `--reps` after a warm-up:
  render_launches_ms   the three launches of t3d_render alone (tables, points, corners and backgrounds already on the device);
  copy_back_ms         the copy of the finished pictures to the host;
  host_spec_ms         tests/fake_render.render_arrays over the first `--host_views` views, scaled to all of them (host_spec_ms_scaled).
The device pictures of the sampled views are compared with the specification's (bytes_differ: the load is random, a point within
rounding of a pixel boundary or of another point's depth is possible; the tests hold the kernel to exact equality on repaired cases).

  python tools/bench_render.py --out profiles/render_bench.json
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from transferable3d_amd import render as R                    # noqa: E402
from transferable3d_amd.engine import Runtime                 # noqa: E402


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), [round(v, 4) for v in t]


def synthetic_views(n_views, H, W, n_points, n_boxes, seed):
    r = np.random.RandomState(seed)
    K = np.array([[529.5, 0, W / 2.0], [0, 529.5, H / 2.0], [0, 0, 1]])
    views = []
    for _ in range(n_views):
        v = R.image_view(np.eye(3), K, H, W, image=r.randint(0, 256, (H, W, 3)).astype(np.uint8))
        xyz = np.stack([r.uniform(-3, 3, n_points), r.uniform(-1.5, 1.5, n_points), r.uniform(0.8, 6, n_points)], 1).astype(np.float32)
        v.points(xyz, rgb=r.uniform(0, 1, (n_points, 3)).astype(np.float32))
        c = np.stack([r.uniform(-2, 2, n_boxes), r.uniform(-0.5, 0.5, n_boxes), r.uniform(2, 5, n_boxes)], 1)
        s = r.uniform(0.3, 1.0, (n_boxes, 3))
        sign = np.array([[1, 1, 1], [1, 1, -1], [-1, 1, -1], [-1, 1, 1], [1, -1, 1], [1, -1, -1], [-1, -1, -1], [-1, -1, 1]], np.float64)
        v.boxes((c[:, None] + 0.5 * s[:, None] * sign[None]).astype(np.float32), [R.CLASS_PALETTE[k % 10] for k in range(n_boxes)], thickness=2)
        views.append(v)
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=16)
    ap.add_argument('--height', type=int, default=530)
    ap.add_argument('--width', type=int, default=730)
    ap.add_argument('--points', type=int, default=50000)
    ap.add_argument('--boxes', type=int, default=20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_views', type=int, default=2, help='views the specification is run over')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import fake_render as FR
    rt = Runtime()
    views = synthetic_views(a.views, a.height, a.width, a.points, a.boxes, a.seed)
    ren = R.Renderer(rt)
    kw, out_bytes = ren.gather(views)
    out = torch.zeros(out_bytes, dtype=torch.uint8, device=rt.device)
    ren.render_tables(out=out, **kw)
    torch.cuda.synchronize()
    launch_ms, launch_all = event_ms(ren.relaunch, a.reps)
    copy_ms, copy_all = event_ms(lambda: out.cpu(), a.reps)
    got = out.cpu().numpy()
    # the specification over the first views, from the same tables
    G = min(a.host_views, a.views)
    col = lambda c: np.array([c[0], c[1], c[2]], np.float32)
    vt, rg, bx = kw['views'][0], kw['ranges'][0], kw['boxes'][0]
    spec_views = [dict(P=np.array(list(vt[i].P), np.float32).reshape(4, 4), w_near=vt[i].w_near, H=vt[i].H, W=vt[i].W, out_offset=vt[i].out_offset,
                       bg_offset=vt[i].bg_offset, bg_colour=col(vt[i].bg_colour)) for i in range(G)]
    ranges = [dict(view=g.view, first=g.first, count=g.count, mode=g.mode, colour0=col(g.colour0), colour1=col(g.colour1), splat=g.splat)
              for g in (rg[i] for i in range(kw['ranges'][1])) if g.view < G]
    boxes = [dict(view=b.view, box=b.box, colour=col(b.colour), thickness=b.thickness) for b in (bx[i] for i in range(kw['boxes'][1])) if b.view < G]
    host = {k: (None if kw[k] is None else kw[k].cpu().numpy()) for k in ('xyz', 'rgb', 'label', 'corners', 'bg')}
    want = np.zeros(out_bytes, np.uint8)
    t0 = time.perf_counter()
    FR.render_arrays(spec_views, host['xyz'], host['rgb'], host['label'], ranges, host['corners'].reshape(-1, 8, 3), boxes, [], want, host['bg'])
    host_ms = (time.perf_counter() - t0) * 1e3
    n = sum(3 * v['H'] * v['W'] for v in spec_views)
    res = dict(views=a.views, height=a.height, width=a.width, points_per_view=a.points, boxes_per_view=a.boxes, reps=a.reps,
               render_launches_ms=round(launch_ms, 4), copy_back_ms=round(copy_ms, 4), host_spec_views=G, host_spec_ms=round(host_ms, 1),
               host_spec_ms_scaled=round(host_ms * a.views / max(G, 1), 1), bytes_differ=[int((got[:n] != want[:n]).sum()), int(n)],
               render_launches_ms_all=launch_all, copy_back_ms_all=copy_all)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
