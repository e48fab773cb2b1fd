"""Generates tests/golden/frustum_scenes.npz + frustum_reference.npz + frustum_reference_flags.json by EXECUTING the reference's frustum
extraction (sunrgbd/sunrgbd_data/sunrgbd_data.py extract_roi_seg and extract_roi_seg_from_rgb_detection, with its utils.py) on small
synthetic SUN-RGBD scenes (run in the build container only, where /root/reference exists: `python tests/golden/make_frustum_vectors.py`).

The reference runs unmodified from where it lies, with placeholder modules as in make_reference_vectors.py: `cv2` (imread decodes with
PIL and returns BGR, what cv2.imread gives) and `cPickle` (the standard pickle).  Its module-level SUNRGBD_DATASET_DIR is pointed at the
scenes written here.  Its os.listdir order of the detection files is made file-name order for the run (the project's one documented
difference).  np.random.random / np.random.choice are wrapped to record the draws of every job; a job is (scene id, ordinal, aug):
the object's line in its label file and the augmentation index, or the detection's position among its image's detections.

Stored: the scenes (depth quantised to 1e-4 as integers, calibration, label and detection lines, the JPEG bytes), the draws, and the
reference's outputs in compact form (per kept frustum the scene-local index of every output point; labels, box2d, box3d, angle, size,
heading, ids, types, img_dims, a digest of the crop).  Before saving, the compact form is checked to rebuild the reference pickles'
arrays exactly.  The generator also asserts the conditions the parity tests rely on: every point's uv lies >= 1e-6 px from every edge
of every (perturbed) 2-D box, and at most 0.1 % of the labelled points lie within 1e-9 m of a 3-D box face.
"""
import ast
import hashlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
REF = '/root/reference/sunrgbd/sunrgbd_data'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_frustum as RF          # noqa: E402

W_IMG, H_IMG = 320, 240
AUGMENT_X = 2
CLASSES = ['bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub']


def fmt(q):
    """an integer count of 1e-4 as the decimal text of a depth file"""
    s = '-' if q < 0 else ''
    q = abs(int(q))
    return '%s%d.%04d' % (s, q // 10000, q % 10000)


def make_scene(rng, sid):
    tilt = rng.uniform(-0.08, 0.08, size=2)
    cx, sx, cy, sy = np.cos(tilt[0]), np.sin(tilt[0]), np.cos(tilt[1]), np.sin(tilt[1])
    rt = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rt = np.round(rt, 6)
    f = rng.uniform(240, 280)
    K = np.array([[round(f, 4), 0, W_IMG / 2.0 + 0.5], [0, round(f, 4), H_IMG / 2.0 - 0.5], [0, 0, 1]])
    n = int(rng.randint(5000, 8000))
    objs, pts = [], []
    # one big object near the camera (its frustum holds > 2048 points), then smaller ones
    for k in range(int(rng.randint(3, 5))):
        big = k == 0
        l, w, h = (rng.uniform(0.7, 1.0), rng.uniform(0.5, 0.8), rng.uniform(0.35, 0.5)) if big else tuple(rng.uniform(0.2, 0.5, size=3))
        c = np.array([rng.uniform(-0.8, 0.8), rng.uniform(2.2, 3.5), rng.uniform(-0.6, 0.2)])
        ang = rng.uniform(-np.pi, np.pi)
        cls = CLASSES[k % 5] if k < 3 else ('lamp' if k == 3 else CLASSES[7])
        m = int(n * (0.55 if big else 0.08))
        # points on and near the box: uniform in a box 5 % larger than the object
        loc = rng.uniform(-1.05, 1.05, size=(m, 3)) * np.array([l, w, h])
        R = np.array([[np.cos(-ang), -np.sin(-ang), 0], [np.sin(-ang), np.cos(-ang), 0], [0, 0, 1]])
        pts.append(loc @ R.T + c)
        objs.append((cls, c, (l, w, h), ang))
    rest = n - sum(len(p) for p in pts)
    pts.append(np.stack([rng.uniform(-2.5, 2.5, rest), rng.uniform(1.0, 6.0, rest), rng.uniform(-1.2, 1.5, rest)], 1))
    xyz = np.concatenate(pts)
    rgb = rng.uniform(0, 1, size=(len(xyz), 3))
    q = np.round(np.concatenate([xyz, rgb], 1) * 1e4).astype(np.int64)
    depth = q / 1e4
    labels = []
    for cls, c, (l, w, h), ang in objs:
        obj = types.SimpleNamespace(heading_angle=-ang, l=l, w=w, h=h, centroid=c)
        ori = (np.cos(ang), np.sin(ang))           # heading_angle = -arctan2(oy, ox) = -ang
        # 2-D box: the projected corners' extent, clipped to the image, whole pixels
        from transferable3d_amd.sunrgbd_data import compute_box_3d, flip_axis_to_camera
        corners_cam = compute_box_3d(types.SimpleNamespace(heading_angle=-ang, l=l, w=w, h=h, centroid=c))
        corners_depth = np.stack([corners_cam[:, 0], corners_cam[:, 2], -corners_cam[:, 1]], 1)
        uv = RF.project_to_image(corners_depth, rt, K)
        x0, y0 = np.clip(np.floor(uv.min(0)), 0, [W_IMG - 1, H_IMG - 1])
        x1, y1 = np.clip(np.ceil(uv.max(0)), 1, [W_IMG, H_IMG])
        labels.append('%s %d %d %d %d %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f'
                      % (cls, x0, y0, x1 - x0, y1 - y0, c[0], c[1], c[2], w, l, h, 1, 0, 0, 1, ori[0], ori[1]))
    dets = []
    for line in labels:
        t = line.split(' ')
        x0, y0, bw, bh = [float(v) for v in t[1:5]]
        j = rng.uniform(-3, 3, size=4)
        dets.append('%s -1 -10 -10 %.2f %.2f %.2f %.2f 0 0 0 0 0 0 0 %.4f' % (t[0], x0 + j[0] + 0.25, y0 + j[1] + 0.25, x0 + bw + j[2] + 0.25,
                                                                                y0 + bh + j[3] + 0.25, rng.uniform(0.05, 0.99)))
    yy, xx = np.mgrid[0:H_IMG, 0:W_IMG]
    img = np.stack([xx * 255.0 / W_IMG, yy * 255.0 / H_IMG, (xx + yy) * 127.0 / (W_IMG + H_IMG) + 40 * sid], 2).astype(np.uint8)
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=75)
    calib = ' '.join('%.6f' % v for v in rt.reshape(-1, order='F')) + '\n' + ' '.join('%.4f' % v for v in K.reshape(-1, order='F')) + '\n'
    return {'depth_q': q, 'calib': calib, 'label': '\n'.join(labels) + '\n', 'det': '\n'.join(dets) + '\n', 'jpeg': buf.getvalue()}


def write_scenes(root, scenes):
    tr = os.path.join(root, 'training')
    for sub in ('image', 'calib', 'depth', 'label_dimension'):
        os.makedirs(os.path.join(tr, sub), exist_ok=True)
    det = os.path.join(root, 'det')
    os.makedirs(det, exist_ok=True)
    for sid, s in scenes.items():
        open(os.path.join(tr, 'calib', '%06d.txt' % sid), 'w').write(s['calib'])
        open(os.path.join(tr, 'label_dimension', '%06d.txt' % sid), 'w').write(s['label'])
        open(os.path.join(det, '%06d.txt' % sid), 'w').write(s['det'])
        open(os.path.join(tr, 'image', '%06d.jpg' % sid), 'wb').write(s['jpeg'])
        with open(os.path.join(tr, 'depth', '%06d.txt' % sid), 'w') as fh:
            fh.write('\n'.join(' '.join(fmt(v) for v in row) for row in s['depth_q']) + '\n')
    return det


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_flags():
    """the reference's argparse flags (name, default, choices), read from its syntax tree"""
    tree = ast.parse(open(os.path.join(REF, 'sunrgbd_data.py')).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, 'attr', '') == 'add_argument':
            kw = {k.arg: ast.literal_eval(k.value) for k in node.keywords if k.arg in ('default', 'choices')}
            out.append({'flag': node.args[0].value, 'default': kw.get('default'), 'choices': kw.get('choices')})
    return out


def main():
    from PIL import Image
    cv2 = types.ModuleType('cv2')
    cv2.imread = lambda p: np.ascontiguousarray(np.asarray(Image.open(p).convert('RGB'))[:, :, ::-1])
    sys.modules['cv2'] = cv2
    import pickle
    sys.modules['cPickle'] = pickle
    utils = load('utils', os.path.join(REF, 'utils.py'))
    sd = load('ref_sunrgbd_data', os.path.join(REF, 'sunrgbd_data.py'))

    rng = np.random.RandomState(11)
    ids = [3, 17, 42]
    scenes = {sid: make_scene(rng, k) for k, sid in enumerate(ids)}
    tmp = tempfile.mkdtemp()
    det = write_scenes(tmp, scenes)
    sd.SUNRGBD_DATASET_DIR = tmp
    idx_file = os.path.join(tmp, 'training', 'idx.txt')
    open(idx_file, 'w').write(''.join('%d\n' % i for i in ids))

    # ---- roi_seg: perturbed boxes, augmentX = 2; record the draws per job
    jobs = []
    for sid in ids:
        for oi, line in enumerate(scenes[sid]['label'].strip().split('\n')):
            if line.split(' ')[0] in sd.__dict__['extract_roi_seg'].__defaults__[-1]:
                jobs += [(sid, oi, a) for a in range(AUGMENT_X)]
    rec = {'perturb': {}, 'choice': {}}
    cur = [None]
    it = iter(jobs)
    real_po, real_rand, real_choice = sd.process_object, np.random.random, np.random.choice

    def po(*a, **k):
        cur[0] = next(it)
        return real_po(*a, **k)

    def rand(*a, **k):
        v = real_rand(*a, **k)
        rec['perturb'].setdefault(cur[0], []).append(float(v))
        return v

    def choice(*a, **k):
        v = real_choice(*a, **k)
        rec['choice'][cur[0]] = np.asarray(v)
        return v
    sd.process_object, np.random.random, np.random.choice = po, rand, choice
    np.random.seed(5)
    out_seg = os.path.join(tmp, 'seg.zip.pickle')
    sd.extract_roi_seg(idx_file, 'training', out_seg, viz=False, perturb_box2d=True, augmentX=AUGMENT_X)
    assert next(it, None) is None
    sd.process_object = real_po

    # ---- detections: sorted listdir; choice draws mapped to the jobs whose frustum exceeds 2048 points
    det_calls = []

    def choice2(n, k, replace=True):
        v = real_choice(n, k, replace=replace)
        det_calls.append((n, np.asarray(v)))
        return v
    np.random.choice, np.random.random = choice2, real_rand
    real_listdir = os.listdir
    os.listdir = lambda p: sorted(real_listdir(p))
    out_det = os.path.join(tmp, 'det.zip.pickle')
    try:
        sd.extract_roi_seg_from_rgb_detection(det, 'training', out_det, viz=False, valid_id_list=None)
    finally:
        os.listdir, np.random.choice = real_listdir, real_choice
    seg = utils.load_zipped_pickle(out_seg)
    dres = utils.load_zipped_pickle(out_det)

    # ---- compact form via the restatement on the recorded draws, checked against the pickles
    from transferable3d_amd.sunrgbd_data import sunrgbd_object, compute_box_3d
    ds = sunrgbd_object(tmp)
    depth = {sid: ds.get_depth(sid) for sid in ids}
    assert all(np.array_equal(depth[s], np.loadtxt(os.path.join(tmp, 'training', 'depth', '%06d.txt' % s))) for s in ids)
    calib = {sid: ds.get_calibration(sid) for sid in ids}
    uv = {sid: RF.project_to_image(depth[sid], calib[sid].Rtilt, calib[sid].K) for sid in ids}
    min_edge, near, labelled = np.inf, 0, 0
    kept = []
    for job in jobs:
        sid, oi, aug = job
        obj = ds.get_label_objects(sid)[oi]
        corners = compute_box_3d(obj)
        r = RF.extract(depth[sid], calib[sid].Rtilt, calib[sid].K, obj.box2d, corners, perturb=rec['perturb'][job], choice=rec['choice'].get(job), uv=uv[sid])
        assert (r['n'] > 2048) == (job in rec['choice'])
        b = r['box2d']
        min_edge = min(min_edge, np.abs(uv[sid][:, 0:1] - b[[0, 2]][None]).min(), np.abs(uv[sid][:, 1:2] - b[[1, 3]][None]).min())
        if np.sum(r['label']) < 5:
            continue
        near += int((RF.face_distance(r['points'], corners) < 1e-9).sum())
        labelled += len(r['points'])
        kept.append((job, r, obj, corners))
    det_jobs, ordinal = [], {}
    for fn in sorted(os.listdir(det)):
        sid = int(fn[:6])
        for line in open(os.path.join(det, fn)):
            t = line.rstrip().split(' ')
            o = ordinal.get(sid, 0)
            ordinal[sid] = o + 1
            if t[0] in CLASSES:
                det_jobs.append(((sid, o, 0), np.array([float(t[i]) for i in range(4, 8)]), t[0], float(t[-1])))
    calls = iter(det_calls)
    det_choice, det_kept = {}, []
    for key, box, cls, prob in det_jobs:
        sid = key[0]
        n = int(RF.extract(depth[sid], calib[sid].Rtilt, calib[sid].K, box, uv=uv[sid], num_points=1 << 30)['n'])
        if n > 2048:
            nn, ch = next(calls)
            assert nn == n
            det_choice[key] = ch
        r = RF.extract(depth[sid], calib[sid].Rtilt, calib[sid].K, box, choice=det_choice.get(key), uv=uv[sid])
        min_edge = min(min_edge, np.abs(uv[sid][:, 0:1] - box[[0, 2]][None]).min(), np.abs(uv[sid][:, 1:2] - box[[1, 3]][None]).min())
        if len(r['points']) >= 5:
            det_kept.append((key, r, box, cls, prob))
    assert next(calls, None) is None
    print('min |uv - box edge| = %.3g px, points within 1e-9 m of a face: %d of %d' % (min_edge, near, labelled))
    assert min_edge >= 1e-6 and near <= 1e-3 * labelled
    assert any(r['n'] > 2048 for _, r, _, _ in kept), 'no frustum is subsampled'

    # the compact form rebuilds the pickles
    assert len(seg[0]) == len(kept) and len(dres[0]) == len(det_kept)
    digest = lambda a: hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()
    for i, (job, r, obj, corners) in enumerate(kept):
        assert seg[0][i] == job[0] and np.array_equal(seg[4][i], r['points']) and np.array_equal(seg[5][i], r['label'])
        assert np.array_equal(seg[1][i], r['box2d']) and np.array_equal(seg[2][i], corners) and seg[6][i] == obj.classname
        assert seg[11][i] == r['frustum_angle'] and seg[7][i] == obj.heading_angle and np.array_equal(seg[8][i], [2 * obj.l, 2 * obj.w, 2 * obj.h])
    for i, (key, r, box, cls, prob) in enumerate(det_kept):
        assert dres[0][i] == key[0] and np.array_equal(dres[3][i], r['points']) and dres[4][i] == cls and dres[6][i] == prob
        assert dres[5][i] == r['frustum_angle'] and np.array_equal(dres[1][i], box)

    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt)
    offs = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    keys_of = lambda d: np.array(list(d.keys()), np.int32).reshape(-1, 3)
    np.savez_compressed(os.path.join(HERE, 'frustum_scenes.npz'), ids=np.array(ids, np.int32),
                        depth_q=np.concatenate([scenes[s]['depth_q'] for s in ids]).astype(np.int32),
                        depth_offsets=offs([scenes[s]['depth_q'] for s in ids]),
                        **{'calib_%d' % s: np.frombuffer(scenes[s]['calib'].encode(), np.uint8) for s in ids},
                        **{'label_%d' % s: np.frombuffer(scenes[s]['label'].encode(), np.uint8) for s in ids},
                        **{'det_%d' % s: np.frombuffer(scenes[s]['det'].encode(), np.uint8) for s in ids},
                        **{'jpeg_%d' % s: np.frombuffer(scenes[s]['jpeg'], np.uint8) for s in ids},
                        augmentX=np.int32(AUGMENT_X),
                        perturb_keys=keys_of(rec['perturb']), perturb=np.array(list(rec['perturb'].values()), np.float64),
                        choice_keys=keys_of(rec['choice']), choice=np.stack(list(rec['choice'].values())).astype(np.int16),
                        det_choice_keys=keys_of(det_choice),
                        det_choice=np.stack(list(det_choice.values())).astype(np.int16) if det_choice else np.zeros((0, 2048), np.int16))
    np.savez_compressed(os.path.join(HERE, 'frustum_reference.npz'),
                        seg_keys=np.array([k[0] for k in kept], np.int32), seg_index=cat([k[1]['index'] for k in kept], np.int16),
                        seg_offsets=offs([k[1]['index'] for k in kept]), seg_label=cat([k[1]['label'] for k in kept], np.uint8),
                        seg_box2d=np.stack([seg[1][i] for i in range(len(kept))]), seg_box3d=np.stack(seg[2]),
                        seg_angle=np.array(seg[11], np.float64), seg_size=np.stack(seg[8]), seg_heading=np.array(seg[7], np.float64),
                        seg_type=np.array(seg[6]), seg_img_dims=np.array(seg[12], np.int32),
                        seg_crop_shape=np.array([c.shape for c in seg[3]], np.int32), seg_crop_sha1=np.array([digest(c) for c in seg[3]]),
                        det_keys=np.array([k[0] for k in det_kept], np.int32), det_index=cat([k[1]['index'] for k in det_kept], np.int16),
                        det_offsets=offs([k[1]['index'] for k in det_kept]), det_box2d=np.stack(dres[1]),
                        det_angle=np.array(dres[5], np.float64), det_type=np.array(dres[4]), det_prob=np.array(dres[6], np.float64),
                        det_crop_shape=np.array([c.shape for c in dres[2]], np.int32), det_crop_sha1=np.array([digest(c) for c in dres[2]]))
    json.dump(reference_flags(), open(os.path.join(HERE, 'frustum_reference_flags.json'), 'w'), indent=1)
    for f in ('frustum_scenes.npz', 'frustum_reference.npz'):
        print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == '__main__':
    main()
