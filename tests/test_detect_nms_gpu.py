"""GPU: t3d_detect_nms (csrc/nms.hip) through nms.DeviceNms against its NumPy fp64 specification (tests/fake_nms.py) on the cases of
tests/nms_check.py -- groups of 1, 2, 63, 64, 65, 130, 260 and 1024 boxes, 40 mixed groups with empty ones and unlisted boxes, score ties,
NaN scores, the chain, identical and zero-volume boxes, both metrics at thresholds 0.25 and 0.5.  keep, suppressed_by and rank are
integers and are compared exactly: the cases keep every same-group IoU 1e-3 away from the threshold (nms_check's margin rule), 50 times
what the device IoU may differ from the specification by.  Then the flow on the golden scenes through libt3d.so."""
import ctypes as C

import numpy as np
import pytest

import nms_check as NC
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu

MOVED = ('mixed_40', 'size_65', 'chain', 'ties_nan', 'size_2', 'zero_volume', 'size_130', 'identical', 'size_1')


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.mark.parametrize('metric,threshold', NC.COMBOS)
def test_kernel_equals_the_spec(rt, metric, threshold):
    for name, c in NC.cases(metric, threshold).items():
        got, want = NC.run_case(rt, c), NC.expected(name, metric, threshold)
        NC.assert_equal(got, want, name)
        listed = [b for g in c.groups for b in g]
        print('%-12s %4d boxes in %2d groups: %d kept, %d suppressed' % (name, c.n, len(c.groups), got[0][listed].sum(), len(listed) - got[0][listed].sum()))


@pytest.mark.parametrize('metric,threshold', [('3d', 0.25), ('bev', 0.5)])
def test_a_group_of_1024(rt, metric, threshold):
    c = NC.big_case(metric, threshold)
    assert [len(g) for g in c.groups] == [abi.DETECT_NMS_MAX_GROUP]
    NC.assert_equal(NC.run_case(rt, c), NC.expected('group_1024', metric, threshold), 'group_1024')


def test_two_runs_give_equal_bytes(rt):
    for name in ('mixed_40', 'size_130', 'size_260', 'ties_nan'):
        c = NC.cases('3d', 0.25)[name]
        a, b = NC.run_case(rt, c), NC.run_case(rt, c)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name


@pytest.mark.parametrize('metric,threshold', [('3d', 0.5), ('bev', 0.25)])
def test_the_same_groups_elsewhere_in_a_larger_call(rt, metric, threshold):
    """Other box indices (interleaved with other groups' boxes and with unlisted ones), the groups in reversed order, rows of three words
    instead of one: per box, the same answers."""
    for k, (name, got) in enumerate(zip(MOVED, NC.moved(rt, MOVED, metric, threshold, seed=3))):
        NC.assert_equal(got, NC.expected(name, metric, threshold), name + ' moved')


def test_unlisted_boxes_keep_what_they_held(rt):
    c = NC.cases('3d', 0.25)['mixed_40']
    keep, sup, rank = NC.run_case(rt, c)
    u = np.asarray(c.unlisted)
    assert len(u) >= 4 and (keep[u] == NC.FILL[0]).all() and (sup[u] == NC.FILL[1]).all() and (rank[u] == NC.FILL[2]).all()
    listed = np.setdiff1d(np.arange(c.n), u)
    assert set(keep[listed]) == {0, 1} and (rank[listed] >= 0).all()
    k = np.stack([NC.corners_of(NC.unit_cube(0.0))] * 3)
    for offsets in ([0], [0, 0, 0]):                            # no group; empty groups only: nothing is launched, nothing written
        got = NC.run(rt, k, np.ones(3, np.float32), offsets, [], 0.25, '3d')
        assert all((g == f).all() for g, f in zip(got, NC.FILL))


def test_a_short_struct_and_a_group_of_1025_are_refused(hip_lib):
    a = abi.DetectNmsArgs()
    a.struct_size -= 8
    assert hip_lib.t3d_detect_nms(C.byref(a), C.c_void_p(0)) == abi.ERR_ABI
    a = abi.DetectNmsArgs(n=2000, n_groups=1, metric=0, max_group=1025)
    assert hip_lib.t3d_detect_nms(C.byref(a), C.c_void_p(0)) == -2


def test_detect_with_nms_equals_the_spec_on_the_plain_run_and_the_two_step_route(rt, tmp_path):
    print('\n'.join(NC.check_flow(rt, tmp_path)))
