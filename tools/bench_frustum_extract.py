"""Frustum extraction timing: 50 synthetic SUN-RGBD scenes of 250 000 points and 10 boxes each, written as files, then
  device   extract_roi_seg through libt3d.so: kernel time per scene (HIP events around each launch) and end to end (parsing included);
  numpy    tests/ref_frustum.py (the reference's per-box NumPy restatement) on the same scenes, parsing excluded.
Writes profiles/frustum_extract_bench.json.  Timing is recorded, not gated.

    python tools/bench_frustum_extract.py [--scenes 50] [--points 250000] [--boxes 10] [--batch 16]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def write_scene(root, sid, depth, rt, K, boxes):
    from PIL import Image
    tr = os.path.join(root, 'training')
    np.savetxt(os.path.join(tr, 'depth', '%06d.txt' % sid), depth, fmt='%.4f')
    with open(os.path.join(tr, 'calib', '%06d.txt' % sid), 'w') as fh:
        fh.write(' '.join(repr(float(v)) for v in rt.reshape(-1, order='F')) + '\n' + ' '.join(repr(float(v)) for v in K.reshape(-1, order='F')) + '\n')
    lines = []
    for k, (box, corners) in enumerate(boxes):
        # a label line whose compute_box_3d gives these corners is not needed for timing: an axis-aligned box around the corners' centre
        c = corners.mean(0)
        lines.append('chair %.2f %.2f %.2f %.2f %.6f %.6f %.6f 0.4 0.4 0.4 1 0 0 1 1 0' % (box[0], box[1], box[2] - box[0], box[3] - box[1],
                                                                                             c[0], c[2], -c[1]))
    open(os.path.join(tr, 'label_dimension', '%06d.txt' % sid), 'w').write('\n'.join(lines) + '\n')
    Image.fromarray(np.full((530, 730, 3), 128, np.uint8)).save(os.path.join(tr, 'image', '%06d.jpg' % sid))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=50)
    ap.add_argument('--points', type=int, default=250000)
    ap.add_argument('--boxes', type=int, default=10)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frustum_extract_bench.json'))
    a = ap.parse_args()
    import frustum_check as FC
    import ref_frustum as RF
    from transferable3d_amd import sunrgbd_data as SD
    from transferable3d_amd.engine import Runtime
    rng = np.random.RandomState(0)
    root = tempfile.mkdtemp()
    for sub in ('image', 'calib', 'depth', 'label_dimension'):
        os.makedirs(os.path.join(root, 'training', sub))
    ids = list(range(a.scenes))
    for s in ids:
        depth, rt, K, boxes = FC.synthetic_scene(rng, n_points=a.points, n_boxes=a.boxes)
        write_scene(root, s, depth, rt, K, boxes)
    rt = Runtime()
    SD.extract_roi_seg(root, ids[:2], rt=rt)                           # warm-up: library, allocator
    timings = []
    t0 = time.perf_counter()
    lists = SD.extract_roi_seg(root, ids, rt=rt, batch_scenes=a.batch, timings=timings)
    e2e = time.perf_counter() - t0
    ds = SD.sunrgbd_object(root)
    scenes = [(ds.get_depth(s), ds.get_calibration(s), ds.get_label_objects(s)) for s in ids]
    t0 = time.perf_counter()
    n_ref = 0
    rs = np.random.RandomState(1)
    for depth, calib, objs in scenes:
        uv = RF.project_to_image(depth, calib.Rtilt, calib.K)
        for obj in objs:
            n = int(RF.extract(depth, calib.Rtilt, calib.K, obj.box2d, uv=uv, num_points=1 << 30)['n'])
            ch = rs.choice(n, 2048, replace=False) if n > 2048 else None
            RF.extract(depth, calib.Rtilt, calib.K, obj.box2d, SD.compute_box_3d(obj), choice=ch, uv=uv)
            n_ref += 1
    ref_s = time.perf_counter() - t0
    res = {'scenes': a.scenes, 'points_per_scene': a.points, 'boxes_per_scene': a.boxes, 'batch_scenes': a.batch,
           'kept_frustums': len(lists[0]), 'device_kernel_ms_per_scene': sum(timings) / a.scenes,
           'device_end_to_end_ms_per_scene': 1e3 * e2e / a.scenes, 'numpy_restatement_ms_per_scene': 1e3 * ref_s / a.scenes,
           'numpy_jobs': n_ref}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
