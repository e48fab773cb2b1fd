"""Shared pieces of the consistency tests (t3d_detect_consistency, consistency.DeviceConsistency, detect --consistency, autolabel): the
kernel-level cases and the launch helper, for tests/test_consistency_cpu.py and tests/test_consistency_gpu.py."""
import numpy as np
import torch

import fake_consistency as FK
from transferable3d_amd import consistency as CS

MARGIN = 1e-9          # see fake_consistency.margins


def box_corners(l, w, h, ry, centre):
    """get_3d_box((l, w, h), ry, centre) -> [8, 3] fp64, in the order t3d_detect_decode writes."""
    x = np.array([l, l, -l, -l, l, l, -l, -l]) / 2.0
    y = np.array([h, h, h, h, -h, -h, -h, -h]) / 2.0
    z = np.array([w, -w, -w, w, w, -w, -w, w]) / 2.0
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([c * x + s * z + centre[0], y + centre[1], -s * x + c * z + centre[2]], 1)


def calib_rows():
    """Two rows of one camera (a SUN-RGBD-like 320 x 240 one, tilted a few degrees): row 0 clips to the image, row 1 does not."""
    a = 0.12
    Rtilt = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    K = np.array([[258.5287, 0.0, 160.5], [0.0, 258.5287, 119.5], [0.0, 0.0, 1.0]])
    return np.stack([CS.calib_row(Rtilt, K, (320, 240)), CS.calib_row(Rtilt, K, None)])


def _points(r, n, k, centre):
    """n points around the box k: uniform in the box's own frame, 1.6 times its size, so that about a quarter lies inside."""
    t = r.uniform(-0.3, 1.3, (n, 3))
    return k[0] + t[:, 0:1] * (k[1] - k[0]) + t[:, 1:2] * (k[3] - k[0]) + t[:, 2:3] * (k[4] - k[0])


def case(seed, B, N, ld=3, with_rot=True):
    """fp32 inputs of the kernel for B detections of N points, rows ld floats apart.  Detection b: b % 5 == 1 has an empty mask, b % 5 == 2
    a full one, every seventh logit pair ties; b % 7 == 3 lies behind the camera; b % 4 == 2 straddles the image border; b % 4 == 0 has
    the 2-D box equal to its own reprojection (IoU exactly 1); detections share two calibration rows and the last one (B >= 3) names a
    row out of range.  Points repeat (the network's draw does).  With rot_angle every point is at least MARGIN (relative to the edge)
    away from every face, redrawn until it is: then the last place of cos / sin cannot flip it (fake_consistency.margins)."""
    r = np.random.RandomState(seed)
    calib = calib_rows()
    corners = np.zeros((B, 8, 3), np.float32)
    xyz = r.normal(0, 1, (B, N, ld)).astype(np.float32)            # (the columns behind the third are never read)
    rot = r.uniform(-1.0, 1.0, B).astype(np.float32) if with_rot else None
    for b in range(B):
        depth = r.uniform(2.0, 5.0) * (-1.0 if b % 7 == 3 else 1.0)
        cx = (0.62 if b % 4 == 2 else r.uniform(-0.25, 0.25)) * abs(depth)
        corners[b] = box_corners(*r.uniform(0.3, 1.5, 3), r.uniform(-np.pi, np.pi), (cx, r.uniform(-0.3, 0.6), depth)).astype(np.float32)
    k64 = corners.astype(np.float64)

    def draw(b, n):
        p = _points(r, n, k64[b], None)
        if rot is not None:                                         # into the frustum's frame: the inverse of the kernel's turn by -rot
            c, s = np.cos(-np.float64(rot[b])), np.sin(-np.float64(rot[b]))
            p = np.stack([c * p[:, 0] + s * p[:, 2], p[:, 1], -s * p[:, 0] + c * p[:, 2]], 1)
        return p.astype(np.float32)

    for b in range(B):
        uniq = max(1, (2 * N) // 3)
        p = draw(b, uniq)
        xyz[b, :, :3] = p[np.arange(N) % uniq]
    if rot is not None:
        for _ in range(20):
            close = ~(FK.margins(xyz, corners, rot) >= MARGIN)
            if not close.any():
                break
            for b, n in zip(*np.nonzero(close)):
                xyz[b, n, :3] = draw(b, 1)[0]
    logits = r.normal(0, 2.0, (B, N, 2)).astype(np.float32)
    logits[:, ::7, 1] = logits[:, ::7, 0]                           # ties: background
    for b in range(B):
        if b % 5 == 1:
            logits[b, :, 0], logits[b, :, 1] = 1.5, -0.5
        if b % 5 == 2:
            logits[b, :, 0], logits[b, :, 1] = -1.0, 2.0
    index = (np.arange(B) % 2).astype(np.int32)
    if B >= 3:
        index[B - 1] = 2 if B % 2 else -1
    box2d = np.zeros((B, 4))
    for b in range(B):
        x0, y0 = r.uniform(0, 200), r.uniform(0, 150)
        box2d[b] = (x0, y0, x0 + r.uniform(20, 150), y0 + r.uniform(20, 120))
        if b % 4 != 3 and 0 <= index[b] < len(calib):               # (b % 4 == 3: a 2-D box drawn without looking at the 3-D one)
            rect, bad = FK.rectangle(corners[b], calib[index[b]])
            if not bad:
                box2d[b] = np.asarray(rect) + (0.0 if b % 4 == 0 else r.uniform(-15, 15, 4))
    return dict(xyz=xyz, logits=logits, corners=corners, rot_angle=rot, box2d=box2d, calib_index=index, calib=calib)


def faces_case():
    """An axis-aligned box with dyadic coordinates, rot_angle NULL: the centres of its six faces and its eight vertices (inside: the box
    is closed), and the six face centres moved 2^-20 outwards (outside).  Every operation of the test is exact here.
    -> (case, expected inside flags [N])."""
    centre, l, w, h = np.array([1.0, 0.5, 3.0]), 2.0, 1.0, 0.5
    k = box_corners(l, w, h, 0.0, centre)
    half = np.array([l, h, w]) / 2.0
    pts, inside = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            d = np.zeros(3)
            d[axis] = sign
            pts += [centre + d * half, centre + d * (half + 2.0 ** -20)]
            inside += [True, False]
    pts += list(k)
    inside += [True] * 8
    pts = np.array(pts)
    N = len(pts)
    logits = np.zeros((1, N, 2), np.float32)
    logits[0, ::2, 1] = 1.0
    c = dict(xyz=pts[None].astype(np.float32), logits=logits, corners=k[None].astype(np.float32), rot_angle=None,
             box2d=np.array([[10.0, 10.0, 100.0, 100.0]]), calib_index=np.zeros(1, np.int32), calib=calib_rows())
    assert np.array_equal(c['xyz'].astype(np.float64), pts[None]) and np.array_equal(c['corners'].astype(np.float64), k[None])
    return c, np.array(inside)


def spec(c, n_valid=None, sentinel=None):
    B = len(c['logits'])
    held = (None, None) if sentinel is None else (np.full((B, 4), sentinel, np.int32), np.full((B, 5), float(sentinel)))
    return FK.consistency(c['xyz'], c['logits'], c['corners'], c['rot_angle'], c['box2d'], c['calib_index'], c['calib'], n_valid=n_valid,
                          counts=held[0], reproj=held[1])


def assert_margin(c):
    """The input condition under which the counts are exact with rot_angle: asserted on the CPU before the launch."""
    if c['rot_angle'] is not None:
        m = FK.margins(c['xyz'], c['corners'], c['rot_angle'])
        assert (m >= MARGIN).all(), 'a point closer than %g to a face: %g' % (MARGIN, np.nanmin(m))


def run_kernel(rt, c, n_valid=None, sentinel=None, pad=0):
    """t3d_detect_consistency through consistency.DeviceConsistency on the case's arrays; `pad`: that many more detections (copies of the
    first) in front of and behind the case.  -> (counts [B, 4] int32, reproj [B, 5] fp64) of the case's rows."""
    assert_margin(c)
    B, N = c['logits'].shape[:2]
    grow = lambda a: np.concatenate([np.repeat(a[:1], pad, 0), a, np.repeat(a[:1], pad, 0)]) if pad else a
    up = lambda k: None if c[k] is None else torch.as_tensor(np.ascontiguousarray(grow(c[k]))).to(rt.device)
    n = B + 2 * pad
    con = CS.DeviceConsistency(rt, n, N, CS.ConsistencyRequest(grow(c['box2d']), c['calib'], grow(c['calib_index'])))
    if sentinel is not None:
        con.counts.fill_(int(sentinel))
        con.reproj.fill_(float(sentinel))
    xyz = up('xyz')
    con.launch(0, n, n if n_valid is None else n_valid, xyz.view(n * N, -1), xyz.shape[2], up('logits'), up('corners'), up('rot_angle'))
    return con.counts.cpu().numpy()[pad:pad + B], con.reproj.cpu().numpy()[pad:pad + B]


# ---- scene-level flow ---------------------------------------------------------------------------------------------------------------
def spec_runtime():
    """A host runtime on the NumPy specification libraries (frustum extraction, the network, decode, NMS, consistency)."""
    import fake_nms as FN
    from fake_detect import DetectDecodeSpec
    from fake_frustum import FakeFrustumLib
    from fake_render import RenderSpec
    from fake_sunrgbd_eval import FakeSunrgbdEvalLib
    from transferable3d_amd.engine import Runtime

    class SpecLib(FK.ConsistencySpec, RenderSpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib, FakeSunrgbdEvalLib):
        pass
    return Runtime(device='cpu', lib=SpecLib())


class Capture:
    """Records what every t3d_detect_consistency launch of a run read on the device (copied to the host before the launch)."""

    def __enter__(self):
        self.batches, self.con = [], None
        self.real = CS.DeviceConsistency.launch
        cap = self

        def launch(con, first, B, n_valid, xyz, ld_xyz, logits, corners, rot_angle=None):
            host = lambda t: None if t is None else t.detach().cpu().numpy().copy()
            cap.con = con
            cap.batches.append(dict(first=first, B=B, n_valid=n_valid, xyz=host(xyz).reshape(-1, ld_xyz)[:B * con.N].reshape(B, con.N, ld_xyz),
                                    logits=host(logits).reshape(-1)[:B * con.N * 2].reshape(B, con.N, 2),
                                    corners=host(corners).reshape(-1)[:B * 24].reshape(B, 8, 3),
                                    rot_angle=None if rot_angle is None else host(rot_angle).reshape(-1)[:B]))
            return cap.real(con, first, B, n_valid, xyz, ld_xyz, logits, corners, rot_angle)
        CS.DeviceConsistency.launch = launch
        return self

    def __exit__(self, *exc):
        CS.DeviceConsistency.launch = self.real

    def spec(self):
        """The specification on what the launches read -> (counts [n, 4], reproj [n, 5]) of the real detections, in order."""
        con = self.con
        box2d, index, calib = con.box2d.cpu().numpy(), con.calib_index.cpu().numpy(), con.calib.cpu().numpy()[:con.n_calib]
        counts, reproj = [], []
        for b in self.batches:
            sl = slice(b['first'], b['first'] + b['B'])
            c = dict(b, box2d=box2d[sl], calib_index=index[sl], calib=calib)
            assert_margin({k: (v[:b['n_valid']] if k in ('xyz', 'corners', 'rot_angle') and v is not None else v) for k, v in c.items()})
            k, r = spec(c, n_valid=b['n_valid'])
            counts.append(k[:b['n_valid']])
            reproj.append(r[:b['n_valid']])
        return np.concatenate(counts), np.concatenate(reproj)


def scenes_with_sizes(root, ids):
    import detect_check as DC
    scenes = DC.load_scenes(root, ids)
    for s, scene in zip(ids, scenes):
        scene['image_wh'] = CS.image_size(str(root / 'training' / 'image' / ('%06d.jpg' % s)))
    return scenes


def check_detector(rt, root):
    """Detector.detect(consistency=True) on the golden scenes with the graph's initial weights: the records' measures equal the
    specification evaluated on what the device held for those detections, bit for bit (the derived ratios are the same fp64 divisions);
    every other field equals that of a run without the option."""
    import detect_check as DC
    from transferable3d_amd import detect as DT
    ids, folder, idx, dets = DC.write_data_set(root)
    scenes = scenes_with_sizes(root, ids)
    flags = lambda: DC.TS.build_flags(DC.MODEL_FLAGS)
    plain = DT.Detector(flags(), rt=rt).detect(scenes, dets, scene_ids=ids)
    lines = []
    with Capture() as cap:
        got = DT.Detector(flags(), rt=rt, consistency=True, log=lines.append).detect(scenes, dets, scene_ids=ids)
    counts, reproj = cap.spec()
    assert (cap.con.calib.cpu().numpy()[:, 18:] == (320.0, 240.0)).all()          # the scenes' image_wh reached the kernel
    flat, flat0 = [r for recs in got for r in recs], [r for recs in plain for r in recs]
    assert len(flat) == len(flat0) == len(counts) > 4 and [len(a) for a in got] == [len(a) for a in plain]
    mib, sbi = CS.derived(counts[:, 0], counts[:, 1], counts[:, 2])
    for i, (r, r0) in enumerate(zip(flat, flat0)):
        assert set(r) == set(r0) | {'reproj_iou', 'reproj_rect', 'mask_in_box', 'seg_box_iou', 'flags'}
        for k in r0:
            assert np.array_equal(r[k], r0[k]), (i, k)
        assert r['reproj_iou'] == reproj[i, 4] and np.array_equal(r['reproj_rect'], reproj[i, :4]) and r['flags'] == counts[i, 3], (i, r, reproj[i])
        assert r['mask_in_box'] == mib[i] and r['seg_box_iou'] == sbi[i], (i, r, counts[i])
    assert any(0 < r['reproj_iou'] < 1 for r in flat) and any(r['flags'] == 0 for r in flat)
    assert lines == ['consistency: kept %d of %d (no threshold)' % (len(flat), len(flat))], lines
    return flat


def check_filter_before_nms(rt, root):
    """One object reported twice (two 2-D boxes a few pixels apart, one group): the worse of the two 3-D boxes by reproj_iou is given the
    better rank.  With NMS alone it suppresses the other; with a threshold between the two values it is rejected before NMS, and the
    other survives."""
    import detect_check as DC
    from transferable3d_amd import detect as DT
    ids, folder, idx, dets = DC.write_data_set(root)
    scenes = scenes_with_sizes(root, ids)[:1]
    name, box, _ = next(d for d in dets[0] if d != DC.SPARSE)
    pair = [tuple(box), tuple(np.asarray(box) + (6.0, 4.0, 6.0, 4.0))]
    run = lambda probs, **kw: DT.Detector(DC.TS.build_flags(DC.MODEL_FLAGS), rt=rt, **kw).detect(
        scenes, [[(name, pair[0], probs[0]), (name, pair[1], probs[1])]], scene_ids=ids[:1])[0]
    both = run((0.9, 0.8), consistency=True)
    assert len(both) == 2
    v = [r['reproj_iou'] for r in both]
    assert v[0] != v[1], v
    worse = int(v[1] < v[0])
    probs = (0.9, 0.8) if worse == 0 else (0.8, 0.9)
    threshold = (v[0] + v[1]) / 2.0
    nms_alone = run(probs, nms_iou=0.05)
    assert len(nms_alone) == 1 and nms_alone[0]['prob'] == 0.9 and np.array_equal(nms_alone[0]['box2d'], pair[worse])      # the other is suppressed
    lines = []
    filtered = run(probs, nms_iou=0.05, min_reproj_iou=threshold, log=lines.append)
    assert len(filtered) == 1 and filtered[0]['prob'] == 0.8 and np.array_equal(filtered[0]['box2d'], pair[1 - worse])    # ... and survives here
    assert filtered[0]['reproj_iou'] == v[1 - worse] >= threshold > v[worse]
    assert lines[0] == 'consistency: kept 1 of 2 (reproj_iou < %g: 1)' % threshold and 'kept 1 of 1' in lines[1], lines
    return v, threshold


def corner_set_distance(a, b):
    """The largest distance from a corner of one box to the nearest corner of the other (two corner sets in any order)."""
    d = np.sqrt(((np.asarray(a)[:, None, :] - np.asarray(b)[None, :, :]) ** 2).sum(-1))
    return max(d.min(0).max(), d.min(1).max())


def check_autolabel(rt, root):
    """autolabel end to end on the golden scenes: OUT with --link_inputs is a data set sunrgbd_data.extract_roi_seg reads, whose box3d
    entries are the accepted boxes within 1e-5 m; evaluate_sunrgbd scores the same predictions, as <class>_pred.txt, against OUT at AP
    100 for every class with an accepted box."""
    import detect_check as DC
    from transferable3d_amd import autolabel as AL, evaluate_sunrgbd as ES, sunrgbd_data as SD
    ids, folder, idx, dets = DC.write_data_set(root)
    classes = sorted(set(d[0] for scene in dets for d in scene))
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--classes'] + classes
    first = AL.main(base + ['--out_dir', str(root / 'auto0')] + DC.MODEL_FLAGS, rt=rt, log=lambda *a: None)
    values = sorted(r['reproj_iou'] for r in first['_records'] if r['detected'])
    threshold = (values[len(values) // 2 - 1] + values[len(values) // 2]) / 2.0          # the lower half is rejected
    out = root / 'auto'
    lines = []
    s = AL.main(base + ['--out_dir', str(out), '--link_inputs', '--score_against_labels', '--min_reproj_iou', repr(threshold)] + DC.MODEL_FLAGS,
                rt=rt, log=lines.append)
    records = s['_records']
    accepted = [r for r in records if r['accepted']]
    n = {k: sum(c[k] for c in s['classes'].values()) for k in ('offered', 'too_few_points', 'accepted', 'rejected')}
    assert n['offered'] == len(records) == n['too_few_points'] + n['accepted'] + n['rejected'] and n['accepted'] == len(accepted)
    assert n['accepted'] >= 2 and n['rejected'] >= 2 and sum(c['rejected_by']['min_reproj_iou'] for c in s['classes'].values()) == n['rejected']
    assert json_equal(str(out / 'autolabel.json'), {k: v for k, v in s.items() if k != '_records'})
    written = [int(l) for l in open(out / 'training' / 'autolabel_idx.txt')]
    assert written == sorted(set(r['image'] for r in accepted)) and all((out / 'training' / sub).is_dir() for sub in ('image', 'calib', 'depth'))
    # read back by sunrgbd_data: one frustum per accepted object, its box3d the accepted box
    lists = SD.extract_roi_seg(str(out), written, type_whitelist=classes, rt=rt, seed=3)
    todo = list(accepted)
    for img, box3d, name in zip(lists[0], lists[2], lists[6]):
        hit = [r for r in todo if r['image'] == img and r['class'] == name and corner_set_distance(box3d, r['corners']) <= 1e-5]
        assert len(hit) >= 1, (img, name)
        todo.remove(hit[0])
    assert len(lists[0]) >= 1 and len(todo) == len(accepted) - len(lists[0])
    assert all(not r['detected'] or r['accepted'] for r in todo) and len(todo) <= len(accepted) // 2      # (a frustum the reread dropped for its points)
    # scored by evaluate_sunrgbd against the labels it wrote
    pred = root / 'pred'
    pred.mkdir()
    for c in ES.CLASS_NAMES['AB']:
        with open(pred / (c + '_pred.txt'), 'w') as fh:
            for r in accepted:
                if r['class'] == c:
                    fh.write('%d %s -1 -1 -10 %f %f %f %f %f %f %f %f %f %f %f %f\n' % ((r['image'], c) + tuple(r['box2d']) + tuple(r['label']) + (1.0,)))
    ap, _ = ES.evaluate(str(pred), str(out), str(out / 'training' / 'autolabel_idx.txt'), 'AB', rt=rt, log=lambda *a: None)
    for c in set(r['class'] for r in accepted):
        assert ap[c] == 1.0, (c, ap)
    assert any('mean 3-D IoU with the label' in l for l in lines)
    return s, threshold


def json_equal(path, want):
    import json
    return json.load(open(path)) == json.loads(json.dumps(want))
