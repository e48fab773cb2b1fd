"""The official SUN-RGBD detection evaluation (transferable3d_amd/evaluate_sunrgbd.py, t3d_sunrgbd_eval) without a GPU: the NumPy
restatement of the MATLAB protocol (tests/ref_sunrgbd_eval.py) and the NumPy specification of the entry point
(tests/fake_sunrgbd_eval.py) on cases whose answers are worked out by hand, the restatement against the rasterised IoU of the oracle,
the parser, the command line and the ABI mirror.  MATLAB is not available: no vector of this protocol is recorded from the reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_sunrgbd_eval as R
import sunrgbd_eval_check as K
from fake_sunrgbd_eval import FakeSunrgbdEvalLib
from transferable3d_amd import abi
from transferable3d_amd import evaluate_sunrgbd as ES
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_rt():
    return Runtime(device='cpu', lib=FakeSunrgbdEvalLib())


def ref_run(det, gt, difficult, threshold):
    return R.compute_pr_curve_3d(det, gt, difficult, threshold)


def spec_run(det, gt, difficult, threshold):
    return ES.compute_pr_curve_3d('chair', det, gt, difficult, threshold, rt=cpu_rt())


def test_hand_derived_overlaps_restatement():
    K.check_hand_overlaps(R.bb3d_overlap_close_form)
    K.check_footprint_invariances(R.bb3d_overlap_close_form)


def test_hand_derived_overlaps_specification_library():
    """The specification library takes its box geometry and its AP from tests/ref_sunrgbd_eval.py: this exercises the host packing, the
    dense-matrix path and the protocol bookkeeping, and is no second opinion on the clip (those are the raster oracle below, for the
    restatement, and the device comparison of tests/test_sunrgbd_eval_gpu.py)."""
    f = lambda a, b: ES.bb3d_overlap_close_form(a, b, rt=cpu_rt())
    K.check_hand_overlaps(f)
    K.check_footprint_invariances(f)


def test_average_precision_worked_by_hand():
    K.check_average_precision(R.get_average_precision)
    K.check_average_precision(ES.get_average_precision)


def test_protocol_cases_restatement():
    K.check_protocol_cases(ref_run)


def test_protocol_cases_specification_library():
    K.check_protocol_cases(spec_run)


def test_restatement_agrees_with_the_rasterised_iou():
    """>= 200 random rotated pairs against oracle/ref_iou_raster.py (no clipping at all), at 1e-4.  box3d_iou_raster takes the centre in
    the camera frame, the size (l, w, h) and the heading; a box struct {centroid (X, Y, Z), coeffs, rotation ry} maps to it by the
    inverse of parse_class_predictions: centre (X, -Z, Y), size 2 * coeffs, heading ry."""
    from oracle.ref_iou_raster import box3d_iou_raster
    r = np.random.RandomState(5)
    n, worst, n_pos = 200, 0.0, 0
    for i in range(n):
        p1 = np.array([r.uniform(-2, 2), r.uniform(2, 5), r.uniform(-1, 1), r.uniform(0.4, 2.5), r.uniform(0.4, 2.5), r.uniform(0.4, 2.0), r.uniform(-np.pi, np.pi)])
        if i < 120:          # near pairs: high overlap, many edge crossings
            p2 = p1 + np.concatenate([r.normal(0, 0.2, 3), np.zeros(3), [r.uniform(-0.6, 0.6)]])
            p2[3:6] = p1[3:6] * r.uniform(0.8, 1.25, 3)
        else:
            p2 = np.array([p1[0] + r.normal(0, 1), p1[1] + r.normal(0, 1), p1[2] + r.normal(0, 0.5), r.uniform(0.4, 2.5), r.uniform(0.4, 2.5), r.uniform(0.4, 2.0),
                           r.uniform(-np.pi, np.pi)])
        mine = R.bb3d_overlap_close_form(K.stack([K.box(*p1)]), K.stack([K.box(*p2)]))[0, 0]
        cam = lambda p: ((p[0], -p[2], p[1]), (p[3], p[4], p[5]), p[6])
        ras = box3d_iou_raster(*cam(p1), *cam(p2), n=2048)[0]
        worst = max(worst, abs(mine - ras))
        n_pos += ras > 0.05
        assert abs(mine - ras) < 1e-4, (i, mine, ras)
    print('restatement against the rasterised IoU: worst |difference| %.2e over %d pairs, %d of them overlapping' % (worst, n, n_pos))
    assert n_pos >= 120


def test_specification_library_equals_the_restatement_on_a_generated_evaluation():
    """Bookkeeping only (rank by counting, per-image ground truth, minimum sorted position, integer scans) against the statement-by-
    statement form: both sides share the restatement's geometry and AP function, so overlaps agree by construction."""
    data = K.generate(seed=3, n_images=60, n_gt=400, n_det=900)
    for c, (det, gt) in data.items():
        ref = R.compute_pr_curve_3d(det, gt, None, 0.25, same_image_only=True)
        got = ES.compute_pr_curve_3d('x', det, gt, None, 0.25, rt=cpu_rt())
        for k in ('isTp', 'isFp', 'isMissed', 'gtAssignment', 'gtIdxAll', 'sortIdx', 'precision', 'recall'):
            assert np.array_equal(ref[k], got[k]), (c, k)
        assert np.abs(ref['maxOverlaps'] - got['maxOverlaps']).max() < 1e-12 and abs(ref['apScore'] - got['apScore']) < 1e-12
        assert 0.05 < got['apScore'] < 0.95 and got['isTp'].sum() > 5 and got['isMissed'].sum() > 0


def test_parser_round_trip_with_test_semisup(tmp_path):
    """write_detection_results -> parse_class_predictions gives the boxes official_predictions builds in memory, to the 6 decimals of the text."""
    from transferable3d_amd import test_semisup as TS
    r = np.random.RandomState(1)
    n = 40
    names = [ES.CLASS_NAMES['AB'][i % 3] for i in range(n)]
    preds = [None, None, None, list(r.normal(size=(n, 3)) + [0, 0, 4]), list(r.randint(0, 12, n)), list(r.uniform(-0.2, 0.2, n)), list(r.randint(0, 10, n)),
             list(r.normal(size=(n, 3)) * 0.1), list(r.uniform(-1, 1, n)), list(r.uniform(-9, 0, n)), None, list(r.randint(1, 20, n)), None, None]
    TS.write_detection_results(str(tmp_path), ES.CLASS_NAMES['AB'], preds, names)
    held = ES.official_predictions(ES.CLASS_NAMES['AB'], preds, names)
    for c in ES.CLASS_NAMES['AB']:
        got = ES.parse_class_predictions(str(tmp_path / (c + '_pred.txt')), c)
        assert len(got['confidence']) == names.count(c) == len(held[c]['confidence'])
        assert np.array_equal(got['image'], held[c]['image'])
        for k in ('centroid', 'coeffs', 'confidence'):
            assert got[k].dtype == np.float64 and np.abs(got[k] - held[c][k]).max(initial=0) <= 1.01e-6, (c, k)      # each a sum of at most two %f fields
        assert np.abs(got['basis'] - held[c]['basis']).max(initial=0) <= 1e-6
    # a line parses to the correctly rounded doubles of its decimal strings
    one = tmp_path / 'x_pred.txt'
    one.write_text('12 chair -1 -1 -10 1.0 2.0 3.0 4.0 0.700000 0.500000 0.900000 0.100000 0.350000 2.300000 0.000000 -1.250000\n\n')
    p = ES.parse_class_predictions(str(one))
    assert p['image'][0] == 12 and p['confidence'][0] == -1.25 and np.array_equal(p['coeffs'][0], [0.9 / 2, 0.5 / 2, 0.7 / 2])
    assert np.array_equal(p['centroid'][0], [0.1, 2.3, 0.7 / 2 - 0.35]) and np.array_equal(p['basis'][0], np.eye(3))
    # a quarter turn: rows (cos ry, -sin ry, 0), (sin ry, cos ry, 0)
    q = ES.boxes_from_label_format([1], [1], [1], [1], [0], [0], [0], [np.pi / 2], [0])
    assert np.allclose(q['basis'][0], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)


def test_prediction_files_missing_empty_and_of_another_class(tmp_path):
    with pytest.raises(FileNotFoundError, match='sofa'):
        ES.parse_class_predictions(str(tmp_path / 'sofa_pred.txt'), 'sofa')
    (tmp_path / 'bed_pred.txt').write_text('')
    assert len(ES.parse_class_predictions(str(tmp_path / 'bed_pred.txt'))['confidence']) == 0
    (tmp_path / 'desk_pred.txt').write_text(K.pred_line(1, 'desk', (0, 4, 0.5), 0.5, 0.5, 0.5, 0.9) + '\n' + K.pred_line(2, 'chair', (0, 4, 0.5), 0.5, 0.5, 0.5, 0.8) + '\n')
    assert len(ES.parse_class_predictions(str(tmp_path / 'desk_pred.txt'))['confidence']) == 2      # the class column is not looked at
    (tmp_path / 'bad_pred.txt').write_text('1 desk 0.5\n')
    with pytest.raises(ValueError, match='17 fields'):
        ES.parse_class_predictions(str(tmp_path / 'bad_pred.txt'))


def test_ground_truth_from_the_label_files(tmp_path):
    pred, data, idx, _ = K.write_cli_data_set(tmp_path)
    gt = ES.benchmark_groundtruth(data, idx)
    assert gt['classname'] == ['table', 'bed', 'sofa', 'sofa', 'night_stand', 'night_stand', 'bookshelf'] and list(gt['image']) == [1, 1, 1, 2, 2, 3, 3]
    sofa = ES.benchmark_groundtruth(data, [1, 2, 3, 4], 'sofa')
    assert list(sofa['image']) == [1, 2] and np.array_equal(sofa['coeffs'], [[0.5, 0.25, 0.5]] * 2) and np.array_equal(sofa['centroid'][0], [-2.0, 4.0, 0.5])
    assert np.array_equal(sofa['basis'][0], np.eye(3))
    # the rectangle sunrgbd_data.compute_box_3d builds (before its axis flip), for a turned box
    from transferable3d_amd import sunrgbd_data as SD
    obj = SD.SUNObject3d(K.label_line('desk', (0.3, 3.0, 0.4), 0.8, 0.3, 0.5, 0.6, -0.8))
    b = ES.boxes_from_label_objects([obj], [1])
    foot = R.get_corners_of_bb3d(b['centroid'][0], b['basis'][0], b['coeffs'][0])[:4, :2]
    want = SD.compute_box_3d(obj)[:, [0, 2]]                       # upright camera (x, -z_depth.., y_depth): columns 0 and 2 are depth x and y
    assert all(np.abs(want - f).sum(1).min() < 1e-12 for f in foot)


def test_command_line_end_to_end(tmp_path):
    pred, data, idx, expected = K.write_cli_data_set(tmp_path)
    lines = []
    ap, mean_ap = ES.main(['--pred_dir', pred, '--dataset_dir', data, '--idx_path', idx, '--test_on', 'B', '--save_curves', str(tmp_path / 'curves')],
                          rt=cpu_rt(), log=lines.append)
    assert lines == expected
    assert ap == {'table': 1.0, 'sofa': 0.5, 'dresser': 0.0, 'night_stand': pytest.approx(5.0 / 6.0, abs=1e-15), 'bookshelf': 0.0}
    z = np.load(str(tmp_path / 'curves' / 'night_stand_pr.npz'))
    assert list(z['isTp']) == [True, False, True, False] and np.array_equal(z['recall'], [0.5, 0.5, 1.0, 1.0]) and set(z.files) == {
        'precision', 'recall', 'isTp', 'isFp', 'maxOverlaps', 'gtAssignment', 'isMissed'}
    assert list(z['gtAssignment']) == [6, 0, 5, 0]                 # indices in the whole ground-truth list, 1-based
    os.remove(os.path.join(pred, 'sofa_pred.txt'))
    with pytest.raises(FileNotFoundError, match='sofa'):
        ES.main(['--pred_dir', pred, '--dataset_dir', data, '--idx_path', idx], rt=cpu_rt(), log=lines.append)
    with pytest.raises(SystemExit):
        ES.main(['--idx_path', idx], rt=cpu_rt())                      # neither --pred_dir nor --official_eval
    with pytest.raises(SystemExit):
        ES.main(['--pred_dir', pred, '--idx_path', idx, '--no_such_flag'], rt=cpu_rt())
    p = ES.parser().parse_args(['--pred_dir', 'd', '--idx_path', 'i'])
    assert (p.test_on, p.threshold, p.dataset_dir, p.gpu, p.save_curves) == ('B', 0.25, 'mysunrgbd', 0, None)


def test_num2str_as_matlab_displays_it():
    assert [ES.num2str(v) for v in (100.0, 0.0, 50.0, 83.33333333333334, 46.666666666666664, 5.123456789, 0.5, float('nan'))] == [
        '100', '0', '50', '83.3333', '46.6667', '5.1235', '0.5', 'NaN']


def test_official_eval_of_a_test_semisup_run_on_the_specification_library(tmp_path):
    K.check_test_semisup_official_eval(cpu_rt(), tmp_path)


def _header_fields(cname):
    import re
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    m = re.search(r'typedef struct \{([^}]*)\}\s*%s;' % cname, h)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.findall(r'(\w+)(?:\[\d+\])?\s*$', part.strip())[0] for part in decl.split(',')]
    return names


def test_ctypes_struct_follows_the_header(tmp_path):
    assert _header_fields('t3d_sunrgbd_eval_args') == [f[0] for f in abi.SunrgbdEvalArgs._fields_]
    src = tmp_path / 's.c'
    src.write_text('#include <stdio.h>\n#include "t3d.h"\nint main(void){printf("%zu %d %llu\\n", sizeof(t3d_sunrgbd_eval_args), '
                   'T3D_V2_SIZE_sunrgbd_eval_args, (unsigned long long)T3D_SUNRGBD_EVAL_WORKSPACE_BYTES(1000, 300));return 0;}\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 's')])
    size, v2, ws = [int(v) for v in subprocess.check_output([str(tmp_path / 's')], text=True).split()]
    assert size == v2 == C.sizeof(abi.SunrgbdEvalArgs) and abi.SunrgbdEvalArgs().struct_size == size
    assert ws == abi.sunrgbd_eval_workspace_bytes(1000, 300)
    assert abi.ENTRY_POINTS['t3d_sunrgbd_eval'][0]._type_ is abi.SunrgbdEvalArgs


def test_a_short_struct_and_missing_arguments_are_refused_without_a_launch():
    lib = abi.load()
    a = abi.SunrgbdEvalArgs()
    a.struct_size -= 8
    assert lib.t3d_sunrgbd_eval(C.byref(a), C.c_void_p(0)) == abi.ERR_ABI
    assert lib.t3d_sunrgbd_eval(C.byref(abi.SunrgbdEvalArgs()), C.c_void_p(0)) == -1
    b = abi.SunrgbdEvalArgs()
    b.P, b.ap = 4, C.cast(C.c_void_p(8), abi.D)
    assert lib.t3d_sunrgbd_eval(C.byref(b), C.c_void_p(0)) == -1          # detections without their arrays
    b.P = -1
    assert lib.t3d_sunrgbd_eval(C.byref(b), C.c_void_p(0)) == -2
    b.P = (1 << 20) + 1                                                   # t3d.h T3D_SUNRGBD_EVAL_MAX_BOXES
    assert lib.t3d_sunrgbd_eval(C.byref(b), C.c_void_p(0)) == -2
