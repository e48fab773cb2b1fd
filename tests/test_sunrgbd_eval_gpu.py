"""GPU: the official SUN-RGBD detection evaluation through libt3d.so (t3d_sunrgbd_eval): the hand-derived and protocol cases of
tests/test_sunrgbd_eval_cpu.py, a generated evaluation at the real scale against the NumPy restatement of the MATLAB files
(tests/ref_sunrgbd_eval.py), bit-reproducibility, and evaluate_sunrgbd --official_eval (a test_semisup run scored from memory).

Tolerance of the two fp64 clips (boundary integral on the device, Sutherland-Hodgman vertex list in the restatement): measured on the
MI355X on the generated evaluation below (docs/EXPERIMENTS.md), MEASURED_WORST is the larger of the worst |max_overlap difference| and
the worst |AP difference|; the bound is 8 times it, capped at 1e-9 -- a larger difference is a bug in one of the two, not rounding."""
import ctypes as C

import numpy as np
import pytest

import ref_sunrgbd_eval as R
import sunrgbd_eval_check as K
from transferable3d_amd import abi
from transferable3d_amd import evaluate_sunrgbd as ES
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu

MEASURED_WORST = 1.099e-14      # |max_overlap difference| of class 8; the worst |AP difference| was 6.7e-16
BOUND = min(8.0 * MEASURED_WORST, 1e-9)


@pytest.fixture
def rt(hip_lib):
    return Runtime(lib=hip_lib)


def test_hand_derived_overlaps_and_invariances(rt):
    f = lambda a, b: ES.bb3d_overlap_close_form(a, b, rt=rt)
    K.check_hand_overlaps(f)
    K.check_footprint_invariances(f)


def test_protocol_cases(rt):
    K.check_protocol_cases(lambda det, gt, difficult, threshold: ES.compute_pr_curve_3d('chair', det, gt, difficult, threshold, rt=rt))


def test_dense_matrix_equals_the_restatement(rt):
    det, gt = K.generate(seed=3, n_images=1, n_gt=60, n_det=80)[0]
    assert len(det['confidence']) > 3 and len(gt['image']) > 3
    got, ref = ES.bb3d_overlap_close_form(det, gt, rt=rt), R.bb3d_overlap_close_form(det, gt)
    print('dense %s: worst |difference| %.3e, %d non-zero' % (got.shape, np.abs(got - ref).max(), (ref != 0).sum()))
    assert (ref != 0).sum() > 10 and np.array_equal(got != 0, ref != 0) and np.abs(got - ref).max() <= BOUND


def test_generated_evaluation_at_the_real_scale_equals_the_restatement(rt):
    """5 000 images, 20 000 boxes, 50 000 detections over ten classes.  No pair is left out: the generator keeps the decisions off the
    boundaries, which is asserted on the restatement's values before anything is compared."""
    data = K.generate(keep_off_boundary=True)
    assert sum(len(d['confidence']) for d, _ in data.values()) == 50000 and sum(len(g['image']) for _, g in data.values()) == 20000
    worst_ov = worst_ap = 0.0
    n_tp = n_pairs = n_ties = 0
    for c, (det, gt) in data.items():
        ref = R.compute_pr_curve_3d(det, gt, None, 0.25, same_image_only=True)
        assert K.off_boundary(ref) == 0, c
        r = ES._eval_call(det, gt, None, 0.25, rt, want_overlaps=True)
        order = r['order'].astype(np.int64)
        d_ov, d_ap = np.abs(r['max_overlap'][order] - ref['maxOverlaps']).max(), abs(float(r['ap'][0]) - ref['apScore'])
        print('class %d: P %d G %d same-image pairs %d tp %d AP %.6f  worst |max_overlap diff| %.3e  |AP diff| %.3e'
              % (c, len(order), len(gt['image']), len(r['overlaps']), int(r['is_tp'].sum()), float(r['ap'][0]), d_ov, d_ap))
        worst_ov, worst_ap = max(worst_ov, d_ov), max(worst_ap, d_ap)
        assert np.array_equal(order, ref['sortIdx']), c
        assert np.array_equal(r['gt_idx'][order], ref['gtIdxAll']), c
        assert np.array_equal(r['is_tp'] != 0, ref['isTp']) and np.array_equal(r['is_fp'] != 0, ref['isFp']), c
        assert np.array_equal(r['is_missed'] != 0, ref['isMissed']) and np.array_equal(r['gt_assignment'], ref['gtAssignment']), c
        assert r['precision'].tobytes() == ref['precision'].tobytes() and r['recall'].tobytes() == ref['recall'].tobytes(), c
        # every same-image entry of allOverlaps
        off = r['overlap_offsets']
        rows = np.repeat(np.arange(len(order)), np.diff(off))
        dense = ref['allOverlaps'][np.argsort(order)]                        # rows back in file order
        assert np.abs(r['overlaps'] - dense[rows, r['overlap_gt']]).max() <= BOUND, c
        assert len(r['overlaps']) == int((det['image'][:, None] == gt['image'][None, :]).sum())
        assert d_ov <= BOUND and d_ap <= BOUND, (c, d_ov, d_ap, BOUND)
        n_tp += int(r['is_tp'].sum()); n_pairs += len(r['overlaps']); n_ties += len(order) - len(np.unique(det['confidence']))
    print('generated evaluation: worst |max_overlap difference| %.3e, worst |AP difference| %.3e, bound %.3e; %d pairs, %d tp, %d tied scores'
          % (worst_ov, worst_ap, BOUND, n_pairs, n_tp, n_ties))
    assert n_tp > 5000 and n_pairs > 50000 and n_ties > 20000


def test_two_runs_give_identical_bytes(rt):
    det, gt = K.generate(seed=8, n_images=300, n_gt=3000, n_det=9000)[4]
    diff = (np.arange(len(gt['image'])) % 7 == 0).astype(np.uint8)
    a = ES._eval_call(det, gt, diff, 0.25, rt, want_overlaps=True)
    b = ES._eval_call(det, gt, diff, 0.25, rt, want_overlaps=True)
    assert set(a) >= {'order', 'max_overlap', 'gt_idx', 'is_tp', 'is_fp', 'gt_assignment', 'is_missed', 'precision', 'recall', 'ap', 'overlaps'}
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    ref = R.compute_pr_curve_3d(det, gt, diff, 0.25, same_image_only=True)   # the "difficult" rule at scale
    assert np.array_equal(a['is_tp'] != 0, ref['isTp']) and np.array_equal(a['is_fp'] != 0, ref['isFp'])
    assert np.array_equal(a['precision'], ref['precision'], equal_nan=True) and np.array_equal(a['recall'], ref['recall'])


def test_official_eval_of_a_test_semisup_run(rt, tmp_path):
    print('\n'.join(K.check_test_semisup_official_eval(rt, tmp_path, num_point=256)))


def test_command_line_on_the_device(rt, tmp_path):
    pred, data, idx, expected = K.write_cli_data_set(tmp_path)
    lines = []
    ES.main(['--pred_dir', pred, '--dataset_dir', data, '--idx_path', idx, '--test_on', 'B'], rt=rt, log=lines.append)
    assert lines == expected


def test_a_short_struct_is_refused(hip_lib):
    a = abi.SunrgbdEvalArgs()
    a.struct_size -= 8
    assert hip_lib.t3d_sunrgbd_eval(C.byref(a), C.c_void_p(0)) == abi.ERR_ABI
