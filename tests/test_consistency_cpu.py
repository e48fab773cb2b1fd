"""CPU: the NumPy fp64 specification of t3d_detect_consistency (tests/fake_consistency.py) against projections the reference itself
computed (tests/golden/consistency_reference.npz), its rectangle / IoU / flag / inclusive-face properties, the auto-label writer's round
trip through sunrgbd_data and evaluate_sunrgbd's ground-truth reader, the counts of autolabel.json, the flags of both command lines, and
the scene-level flows (Detector.detect(consistency=True), the filter in front of NMS, autolabel end to end) on the specification libraries."""
import ctypes as C
import os

import numpy as np
import pytest

import consistency_check as CC
import fake_consistency as FK
from transferable3d_amd import abi, autolabel as AL, consistency as CS, detect as DT, evaluate_sunrgbd as ES, semisup_infer as SI
from transferable3d_amd import sunrgbd_data as SD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# |pixel values| <= 1e4 (a box next to the camera plane reaches a few thousand), fewer than 20 roundings of 2^-53 relative each between
# the corners and a pixel coordinate: 2^-53 * 1e4 * 20 ~ 2e-11.  The reference's BLAS may order the three-term sums differently.
PROJECTION_BOUND = 1e-9


@pytest.fixture(scope='module')
def rt():
    return CC.spec_runtime()


def test_spec_reproduces_the_references_projections():
    V = np.load(os.path.join(GOLDEN, 'consistency_reference.npz'))
    assert len(V['uv']) >= 40 and set(V['kind']) == {0, 1, 2} and np.abs(V['uv']).max() <= 1e4
    worst = 0.0
    for i in range(len(V['uv'])):
        cam = SD.flip_axis_to_camera(V['corners_depth'][i])                  # project_upright_depth_to_upright_camera
        u, v, depth = FK.project(cam, CS.calib_row(V['Rtilt'][i], V['K'][i]))
        worst = max(worst, np.abs(u - V['uv'][i][:, 0]).max(), np.abs(v - V['uv'][i][:, 1]).max(), np.abs(depth - V['depth'][i]).max())
        rect, bad = FK.rectangle(cam.astype(np.float32), CS.calib_row(V['Rtilt'][i], V['K'][i], (320, 240)))
        assert bad == (V['kind'][i] == 2)                                    # behind the camera: flagged
        if V['kind'][i] == 1:                                                # across the border: clipped to it
            assert rect[0] == 0.0 or rect[2] == 319.0
            assert V['uv'][i][:, 0].min() < 0 or V['uv'][i][:, 0].max() > 319
    print('worst |spec - reference| over %d boxes: %.3e (bound %.1e)' % (len(V['uv']), worst, PROJECTION_BOUND))
    assert worst <= PROJECTION_BOUND


def test_rectangle_and_iou_properties():
    a = (10.0, 20.0, 110.0, 70.0)
    assert FK.rect_iou(a, a) == 1.0
    assert FK.rect_iou(a, (110.0, 20.0, 150.0, 70.0)) == 0.0 and FK.rect_iou(a, (200.0, 200.0, 250.0, 250.0)) == 0.0      # touching, apart
    assert FK.rect_iou(a, (60.0, 20.0, 160.0, 70.0)) == 2500.0 / 7500.0
    assert FK.rect_iou((5.0, 5.0, 5.0, 5.0), (5.0, 5.0, 5.0, 5.0)) == 0.0                                                 # no area: 0, not NaN
    cal = CC.calib_rows()
    k = CC.box_corners(1.0, 0.8, 0.6, 0.3, (2.2, 0.2, 3.0)).astype(np.float32)               # across the right border
    clipped, _ = FK.rectangle(k, cal[0])
    free, _ = FK.rectangle(k, cal[1])
    assert free[2] > 319.0 and clipped[2] == 319.0 and clipped[0] == free[0] and 0.0 <= clipped[1] <= clipped[3] <= 239.0
    out = FK.rectangle(CC.box_corners(1.0, 0.8, 0.6, 0.3, (40.0, 0.2, 3.0)).astype(np.float32), cal[0])[0]      # all of it outside: collapses
    assert out[0] == out[2] == 319.0 and FK.rect_iou(out, a) == 0.0


def test_each_flag_is_raised_in_its_case():
    c = CC.case(3, 8, 40, 3, False)
    counts, reproj = CC.spec(c)
    flags = counts[:, 3]
    assert flags[1] & FK.EMPTY_MASK and counts[1, 0] == 0 and not flags[0] & FK.EMPTY_MASK
    assert flags[3] & FK.BAD_PROJECTION and (reproj[3] == 0).all() and not flags[0] & FK.BAD_PROJECTION
    assert flags[7] & FK.NO_CALIB and (reproj[7] == 0).all() and counts[7, 1] > 0 and ((flags & FK.NO_CALIB) != 0).sum() == 1
    assert reproj[0, 4] == 1.0 and counts[2, 0] == 40
    mib, sbi = CS.derived(counts[:, 0], counts[:, 1], counts[:, 2])
    assert mib[1] == 0.0 and sbi[2] == counts[2, 2] / (40 + counts[2, 1] - counts[2, 2]) and ((0 <= mib) & (mib <= 1)).all()
    c['corners'][4] = np.nan                                                    # a NaN anywhere: not inside, a bad projection
    counts, reproj = CC.spec(c)
    assert counts[4, 1] == 0 and counts[4, 3] & FK.BAD_PROJECTION and (reproj[4] == 0).all()
    kept = CC.spec(c, n_valid=3, sentinel=-9)
    assert (kept[0][3:] == -9).all() and (kept[1][3:] == -9.0).all() and (kept[0][:3] == counts[:3]).all()


def test_faces_and_vertices_are_inside():
    c, inside = CC.faces_case()
    counts, _ = CC.spec(c)
    dv, dd = FK.edge_terms(c['xyz'], c['corners'], None)
    assert np.array_equal(np.all((0.0 <= dv) & (dv <= dd), axis=0)[0], inside) and inside.sum() == 14 and (~inside).sum() == 6
    mask = c['logits'][0, :, 1] > c['logits'][0, :, 0]
    assert list(counts[0, :3]) == [mask.sum(), 14, (mask & inside).sum()]


def test_spec_library_entry_point_refuses_what_the_header_says(rt):
    a = abi.DetectConsistencyArgs()
    assert rt.lib.t3d_detect_consistency(C.byref(a), None) == -2
    a.struct_size -= 8
    assert rt.lib.t3d_detect_consistency(C.byref(a), None) == abi.ERR_ABI
    c = CC.case(4, 3, 65, 4, True)
    got = CC.run_kernel(rt, c, n_valid=2, sentinel=-3)                          # DeviceConsistency on host buffers
    want = CC.spec(c, n_valid=2, sentinel=-3)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def decoded_rows(n, seed=5):
    r = np.random.RandomState(seed)
    return np.stack([r.uniform(0.3, 2.0, n), r.uniform(0.3, 2.0, n), r.uniform(0.3, 2.5, n), r.uniform(-3, 3, n), r.uniform(-1, 1.5, n),
                     r.uniform(1, 8, n), r.uniform(-np.pi, np.pi, n)], 1)


def test_label_lines_read_back_as_the_decoded_boxes(tmp_path):
    """decoded rows -> lines -> read_sunrgbd_label + compute_box_3d: the decode's corner sets within 1e-5 m (six decimals of %f on
    coordinates and half sizes, a box below 3 m: 0.5e-6 * (1 + 1.5 + 1.5 + ...) < 1e-5); evaluate_sunrgbd's ground-truth reader
    gives the box its prediction reader gives for the same row."""
    rows = decoded_rows(200)
    path = tmp_path / 'labels.txt'
    box2d = [(10.4, 20.6, 110.5, 90.2)] * len(rows)
    path.write_text(''.join(AL.label_line('table', b, row) + '\n' for b, row in zip(box2d, rows)))
    objs = SD.read_sunrgbd_label(str(path))
    assert len(objs) == len(rows) and all(len(l.split(' ')) == 17 for l in path.read_text().splitlines())
    assert list(objs[0].box2d) == [10.0, 21.0, 110.0, 91.0]                      # x, y, w, h as integers
    from transferable3d_amd.eval_det import get_3d_box
    worst = 0.0
    for o, (h, w, l, tx, ty, tz, ry) in zip(objs, rows):
        want = get_3d_box((l, w, h), ry, (tx, ty - h / 2.0, tz))
        worst = max(worst, CC.corner_set_distance(SD.compute_box_3d(o), want), CC.corner_set_distance(AL.label_corners(o), want))
    print('worst corner distance after the text round trip: %.3e' % worst)
    assert worst <= 1e-5
    gt = ES.boxes_from_label_objects(objs, np.arange(len(objs)))
    pred = ES.boxes_from_label_format(np.arange(len(rows)), *rows.T, np.ones(len(rows)))
    for k in ('centroid', 'basis', 'coeffs'):
        assert np.abs(gt[k] - pred[k]).max() <= 1e-5, k


def test_autolabel_counts_on_injected_records():
    rec = lambda cls, detected=True, accepted=False, v=(0.9, 0.9, 0.9): dict({'class': cls, 'detected': detected, 'accepted': accepted},
                                                                            **dict(zip(CS.MEASURES, v)))
    records = [rec('table', accepted=True), rec('table', v=(0.1, 0.9, 0.9)), rec('table', v=(0.1, 0.2, 0.9)), rec('table', detected=False),
               rec('sofa', accepted=True), rec('sofa', v=(0.9, 0.9, float('nan')))]
    got = AL.count(records, ['table', 'sofa', 'desk'], SI.active_tests(CS.ConsistencyRequest(np.zeros((0, 4)), np.zeros((0, 20)), [], 0.5, 0.5, None)))
    assert dict(got['table']) == {'offered': 4, 'too_few_points': 1, 'accepted': 1, 'rejected': 2,
                                  'rejected_by': {'min_reproj_iou': 2, 'min_mask_in_box': 1}}
    assert got['sofa']['accepted'] == 1 and got['sofa']['rejected'] == 1 and got['desk']['offered'] == 0
    assert 'min_seg_box_iou' not in got['table']['rejected_by']
    accept, below = CS.accept_of(np.array([0.9, 0.1, 0.1]), np.array([0.9, 0.9, 0.2]), np.array([0.9, 0.9, np.nan]), (0.5, 0.5, None))
    assert list(accept) == [True, False, False] and below == {'min_reproj_iou': 2, 'min_mask_in_box': 1}
    assert CS.log_line(accept, below, (0.5, 0.5, None)) == 'consistency: kept 1 of 3 (reproj_iou < 0.5: 2, mask_in_box < 0.5: 1)'


def test_flag_validation():
    for bad in (-0.1, 1.5, float('nan')):
        for name in CS.THRESHOLDS:
            with pytest.raises(ValueError):
                CS.check_thresholds(**{name: bad})
            with pytest.raises(SystemExit):
                DT.main(['--idx_path', 'x', '--rgb_detection_path', 'y', '--' + name, repr(bad)])
            with pytest.raises(SystemExit):
                AL.parse(['--idx_path', 'x', '--classes', 'table', '--out_dir', 'o', '--' + name, repr(bad)])
    assert CS.check_thresholds(0, 1, None) == (0.0, 1.0, None)
    with pytest.raises(SystemExit):
        DT.main(['--idx_path', 'x', '--rgb_detection_path', 'y', '--consistency_json', 'f.json'])      # needs --consistency
    with pytest.raises(SystemExit):
        AL.parse(['--idx_path', 'x', '--out_dir', 'o'])                                                 # --classes is required
    args, flags = AL.parse(['--idx_path', 'x', '--classes', 'table', 'sofa', '--out_dir', 'o', '--min_seg_box_iou', '0.25', '--num_point', '512',
                            '--link_inputs'])
    assert args.thresholds == (None, None, 0.25) and args.classes == ['table', 'sofa'] and flags.num_point == 512 and args.link_inputs
    a = DT.parser().parse_known_args(['--idx_path', 'x', '--rgb_detection_path', 'y', '--min_mask_in_box', '0.5'])[0]
    assert a.min_mask_in_box == 0.5 and not a.consistency and a.consistency_json is None
    with pytest.raises(ValueError):
        SI.inference(None, None, None, None, 4, decode='host', consistency=CS.ConsistencyRequest(np.zeros((1, 4)), np.zeros((1, 20)), [0]))
    with pytest.raises(ValueError):
        CS.ConsistencyRequest(np.zeros((2, 4)), np.zeros((1, 20)), [0])


def test_detector_measures_equal_the_spec_on_what_the_device_held(rt, tmp_path):
    CC.check_detector(rt, tmp_path)


def test_a_rejected_box_does_not_suppress_a_good_one(rt, tmp_path):
    print(CC.check_filter_before_nms(rt, tmp_path))


def test_autolabel_end_to_end(rt, tmp_path):
    s, threshold = CC.check_autolabel(rt, tmp_path)
    print({c: dict(v) for c, v in s['classes'].items()}, threshold)


def test_detect_command_line_with_and_without_the_flags(rt, tmp_path):
    """detect --consistency writes the result files of the plain run byte for byte (nothing is rejected without a threshold) plus the JSON
    rows; with a threshold the rejected detections' lines are gone and nothing else changes."""
    import json
    import detect_check as DC
    ids, folder, idx, dets = DC.write_data_set(tmp_path)
    base = ['--dataset_dir', str(tmp_path), '--idx_path', idx, '--rgb_detection_path', folder]
    run = lambda name, extra: DT.main(base + ['--result_dir', str(tmp_path / name)] + extra + DC.MODEL_FLAGS, rt=rt, log=lambda *a: None)
    run('plain', [])
    js = tmp_path / 'c.json'
    run('measured', ['--consistency', '--consistency_json', str(js)])
    plain = DC.read_results(str(tmp_path / 'plain'))
    assert DC.read_results(str(tmp_path / 'measured')) == plain
    rows = json.load(open(js))
    n = sum(len(t.splitlines()) for t in plain.values())
    assert len(rows) == n and all(r['accepted'] and r['kept'] for r in rows) and all(0.0 <= r['reproj_iou'] <= 1.0 for r in rows)
    assert all(0.0 <= r['reproj_rect'][0] <= r['reproj_rect'][2] <= 319.0 and 0.0 <= r['reproj_rect'][1] <= r['reproj_rect'][3] <= 239.0 for r in rows)
    values = sorted(r['mask_in_box'] for r in rows)
    t = (values[0] + values[-1]) / 2.0
    run('filtered', ['--min_mask_in_box', repr(t), '--consistency_json', str(js)])
    rows = json.load(open(js))
    rejected = [r for r in rows if not r['accepted']]
    assert len(rows) == n and 0 < len(rejected) < n and all((r['mask_in_box'] < t) == (not r['accepted']) for r in rows)
    filtered = DC.read_results(str(tmp_path / 'filtered'))
    assert sum(len(v.splitlines()) for v in filtered.values()) == n - len(rejected)
    for c, text in plain.items():
        assert set(filtered.get(c, '').splitlines()) <= set(text.splitlines())


def test_fed_frustums_are_measured_as_they_stand(rt):
    """inference(decode='device', consistency=...) on frustums fed from the host (no rot_angle: the points are used as they stand): the
    Decoded fields equal the specification on what the launches read, and slicing carries them."""
    import detect_check as DC
    flags = DC.TS.build_flags(DC.MODEL_FLAGS)
    B, N = flags.batch_size, flags.num_point
    sess, ops = DC.TS.get_model(flags, B, N, flags.NUM_CHANNELS, rt=rt)
    r = np.random.RandomState(6)
    n = 2 * B
    pc = r.normal(0, 1, (n, N, flags.NUM_CHANNELS)).astype(np.float32)
    pc[:, :, 2] += 3.0
    one_hot = np.eye(10, dtype=np.float32)[r.randint(0, 10, n)]
    cal = CC.calib_rows()
    req = CS.ConsistencyRequest(r.uniform(0, 200, (n, 4)) + (0, 0, 100, 100), cal, np.arange(n) % 2, min_mask_in_box=0.5)
    with CC.Capture() as cap:
        res = SI.inference(sess, ops, pc, one_hot, B, prefix=flags.pred_prefix, decode='device', consistency=req)
    d = res.decoded
    assert len(cap.batches) == 2 and all(b['rot_angle'] is None for b in cap.batches) and d.keep is None
    assert np.array_equal(np.concatenate([b['xyz'][:, :, :3] for b in cap.batches]), pc[:, :, :3])
    counts, reproj = cap.spec()
    assert np.array_equal(np.stack([d.n_mask, d.n_box, d.n_both, d.flags], 1), counts) and np.array_equal(d.mask_count, d.n_mask)
    assert np.array_equal(d.reproj_rect, reproj[:, :4]) and np.array_equal(d.reproj_iou, reproj[:, 4])
    assert np.array_equal(d.accept, d.mask_in_box >= 0.5) and np.array_equal(d[3:5].accept, d.accept[3:5]) and d[3:5].reproj_rect.shape == (2, 4)
    assert SI.inference(sess, ops, pc, one_hot, B, prefix=flags.pred_prefix, decode='device').decoded.accept is None


def test_vis_legends_carry_the_numbers(rt, tmp_path):
    import json
    import detect_check as DC
    ids, folder, idx, dets = DC.write_data_set(tmp_path)
    det = DT.Detector(DC.TS.build_flags(DC.MODEL_FLAGS), rt=rt, consistency=True)
    records = det.detect(CC.scenes_with_sizes(tmp_path, ids), dets, scene_ids=ids, vis_dir=str(tmp_path / 'vis'), vis_max=1)
    legend = json.load(open(tmp_path / 'vis' / ('%06d.json' % ids[0])))
    boxes = [b for b in legend['boxes'] if b['kind'] == 'kept']
    assert len(boxes) == len(records[0]) > 0
    for b, r in zip(boxes, records[0]):
        assert b['reproj_iou'] == r['reproj_iou'] and b['mask_in_box'] == r['mask_in_box'] and b['flags'] == r['flags'] and len(b['reproj_rect']) == 4
