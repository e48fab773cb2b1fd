"""GPU: the threshold sweep through libt3d.so (csrc/nms_sweep.hip, csrc/sunrgbd_sweep.hip) on the cases of tests/sweep_check.py.  The
reference of every configuration is the EXISTING kernel run on that configuration alone -- t3d_detect_nms on the restricted lists,
t3d_sunrgbd_eval on the selected detections -- so the suppression is compared byte for byte with no margin around the thresholds (the
same fp32 IoU decides in both), the counts of the evaluation exactly, and its AP within 1e-12: the two sums hold the same at most P
non-negative terms, totalling at most 1, in different fixed orders, and P * 2^-52 < 6e-13 at P = 2500."""
import ctypes as C

import numpy as np
import pytest

import fake_sweep as FS
import nms_check as NC
import sweep_check as SW
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.fixture(scope='module')
def sizes():
    return SW.nms_case()


# ---- t3d_detect_nms_sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', NC.METRICS)
@pytest.mark.parametrize('M,K', [(1, 1), (3, 4), (17, 1), (17, 4)])
def test_rows_equal_one_nms_call_per_configuration(rt, sizes, metric, M, K):
    """Groups of 0, 1, 2, 63, 64, 65 and 130 boxes and boxes in no group, n no multiple of 64; thresholds 0, 0.25, 0.5, 1 and the index -1;
    rows of ones, of zeros and random ones; n_kept exact."""
    keep, n_kept, ct, listed = SW.check_nms_sweep(rt, sizes, M, K, metric)
    assert M < 3 or (n_kept[0] > n_kept[2] > 0 == n_kept[1])
    SW.check_nms_sweep(rt, sizes, M, K, metric, with_listed=False)          # listed == NULL: every box, in every configuration


@pytest.mark.parametrize('metric', NC.METRICS)
def test_a_group_of_1024(rt, metric):
    case = SW.big_nms_case()
    assert max(len(g) for g in case.groups) == abi.DETECT_NMS_MAX_GROUP
    keep, n_kept, _, _ = SW.check_nms_sweep(rt, case, 5, 4, metric)
    assert 256 <= n_kept[3] < 1027                                          # all listed, above 0.5: copies are suppressed, every object stays


def test_two_runs_give_equal_bytes_and_the_groups_answer_wherever_they_sit(rt, sizes):
    for metric in NC.METRICS:
        a = SW.check_nms_sweep(rt, sizes, 17, 4, metric, seed=3)
        b = SW.check_nms_sweep(rt, sizes, 17, 4, metric, seed=3)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert SW.moved_nms_sweep(rt, sizes, 17, 4, metric, seed=3).tobytes() == a[0].tobytes()


@pytest.mark.parametrize('metric', NC.METRICS)
def test_the_kernel_equals_the_fp64_specification_off_the_thresholds(rt, metric):
    """The one comparison with the fp64 specification: on a case redrawn until no same-group IoU lies within nms_check.MARGIN of any
    threshold of the grid (sweep_check.repaired_case; no case is left out)."""
    thresholds = SW.GRID_K[4]
    case = SW.repaired_case(metric, thresholds)
    corners, score, offsets, members = case.arrays()
    ct, listed = SW.configs(9, 4, case.n, seed=1)
    keep, n_kept = SW.run_nms_sweep(rt, corners, score, offsets, members, thresholds, ct, listed, metric)
    want, want_n = FS.nms_sweep(corners, score, offsets, members, thresholds, ct, listed, NC.METRIC_ID[metric])
    assert keep.tobytes() == want.tobytes() and np.array_equal(n_kept, want_n)


def test_empty_calls_and_refusals(rt, hip_lib):
    k = np.stack([NC.corners_of(NC.unit_cube(0.0))] * 3)
    for offsets in ([0], [0, 0, 0]):
        keep, n_kept = SW.run_nms_sweep(rt, k, np.ones(3, np.float32), offsets, [], [0.5], [0, -1], None, '3d')
        assert keep.shape == (2, 3) and not keep.any() and list(n_kept) == [0, 0]
    a = abi.DetectNmsSweepArgs()
    a.struct_size -= 8
    assert hip_lib.t3d_detect_nms_sweep(C.byref(a), C.c_void_p(0)) == abi.ERR_ABI
    assert hip_lib.t3d_detect_nms_sweep(C.byref(abi.DetectNmsSweepArgs(n=2000, n_groups=1, max_group=1025, M=1, n_thresholds=1)), C.c_void_p(0)) == -2


# ---- t3d_sunrgbd_eval_sweep -----------------------------------------------------------------------------------------------------------
# EV_CURVE_THREADS = 1024: P = 1023, 1024, 1025 lie on both sides of one detection per thread, 2500 gives uneven chunks of 3
@pytest.mark.parametrize('P,G,M,wide', [(0, 0, 1, False), (0, 40, 5, False), (1, 1, 1, False), (1, 0, 5, True), (1023, 40, 5, False),
                                          (1024, 1, 33, True), (1025, 40, 33, False), (2500, 40, 5, True), (2500, 1, 33, False), (2500, 0, 5, False)])
def test_rows_equal_one_evaluation_per_configuration(rt, P, G, M, wide):
    """Tied and NaN confidences, detections in images without ground truth, det_index NULL and a permutation into a wider matrix, rows of
    ones, of zeros and random ones: n_det, n_tp, n_fp exactly those of a t3d_sunrgbd_eval call on the subset alone, ap within 1e-12, the
    row of ones the bytes of eval->ap, every output of the evaluation the bytes of a plain call, two runs equal bytes."""
    print(SW.check_eval_sweep(rt, P, G, M, wide=wide))


# ---- detect --sweep -------------------------------------------------------------------------------------------------------------------
def test_detect_sweep_equals_one_detect_run_per_row(rt, tmp_path):
    print('\n'.join(SW.check_flow(rt, tmp_path, exact=False)))
