"""GPU: t3d_detect_soft_nms (csrc/soft_nms.hip) through nms.DeviceSoftNms against its NumPy fp64 specification (tests/fake_soft_nms.py) on
the cases of tests/soft_nms_check.py -- groups of 1, 2, 63, 64, 65, 130, 260 and 1024 boxes, 40 mixed groups with empty ones and unlisted
boxes, score ties, scores that take no part, the chain, identical and zero-volume boxes -- under the four passes (metric, method,
threshold, sigma, floor) of soft_nms_check.PASSES.  keep, suppressed_by and n_decays are compared exactly, score_out within twice the bound it accumulates for an IoU error of 2e-5; the cases hold no decision inside
that bound.  Then the equality with t3d_detect_nms where every decay prunes, determinism, locality, and the flow through libt3d.so."""
import ctypes as C

import numpy as np
import pytest

import nms_check as NC
import soft_nms_check as SC
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu

MOVED = ('mixed_40', 'size_65', 'chain', 'ties_nan', 'size_2', 'zero_volume', 'size_130', 'identical', 'size_1')
PASS_IDS = range(len(SC.PASSES))


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.mark.parametrize('pass_id', PASS_IDS)
def test_kernel_equals_the_spec(rt, pass_id):
    for name, c in SC.cases(pass_id).items():
        SC.check_case(SC.run_case(rt, c), c)


@pytest.mark.parametrize('pass_id', SC.BIG_PASSES)
def test_a_group_of_1024(rt, pass_id):
    c = SC.big_case(pass_id)
    assert [len(g) for g in c.groups] == [abi.DETECT_NMS_MAX_GROUP]
    SC.check_case(SC.run_case(rt, c), c)


@pytest.mark.parametrize('metric,threshold', [('3d', 0.25), ('bev', 0.5)])
def test_linear_with_a_floor_above_every_score_is_t3d_detect_nms(rt, metric, threshold):
    """Consequence (a) on the device, byte for byte: both kernels take IoU(better box, other box) from the same function."""
    for name, c, t in [(n, c, threshold) for n, c in NC.cases(metric, threshold).items()] + [('group_1024', NC.big_case(metric, 0.25), 0.25)]:
        k, s, off, mem = c.arrays()
        soft = SC.run_with(rt, k, s, off, mem, 'linear', t, None, 2.0, metric)
        SC.hard_equal(soft, NC.run(rt, k, s, off, mem, t, metric), s, mem, name)
        assert soft[3][mem].max(initial=0) <= 1


def test_two_runs_give_equal_bytes(rt):
    for pass_id in (0, 3):
        for name in ('mixed_40', 'size_130', 'size_260', 'ties_nan'):
            c = SC.cases(pass_id)[name]
            a, b = SC.run_case(rt, c), SC.run_case(rt, c)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name


@pytest.mark.parametrize('pass_id', (1, 2))
def test_the_same_groups_elsewhere_in_a_larger_call(rt, pass_id):
    """Other box indices (interleaved with other groups' boxes and with unlisted ones), the groups in reversed order, 64 lanes per group
    where the case alone has fewer: per box, the bytes of the call that holds the case alone (suppressed_by through the permutation)."""
    for name, got in zip(MOVED, SC.moved(rt, MOVED, pass_id, seed=3)):
        c = SC.cases(pass_id)[name]
        alone = SC.run(rt, *c.arrays(), pass_id)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, alone)), name
        SC.check_case(got, c, name + ' moved', want=c.want_at_pass_floor)


def test_unlisted_boxes_keep_what_they_held(rt):
    c = SC.cases(1)['mixed_40']
    got = SC.run_case(rt, c)
    u = np.asarray(c.c.unlisted)
    assert len(u) >= 4 and all((g[u] == f).all() for g, f in zip(got, SC.FILL))
    listed = np.setdiff1d(np.arange(c.n), u)
    assert set(got[1][listed]) == {0, 1} and (got[3][listed] >= 0).all()
    k = np.stack([NC.corners_of(NC.unit_cube(0.0))] * 3)
    for offsets in ([0], [0, 0, 0]):                            # no group; empty groups only: nothing is launched, nothing written
        got = SC.run(rt, k, np.ones(3, np.float32), offsets, [], 0)
        assert all((g == f).all() for g, f in zip(got, SC.FILL))


def test_a_short_struct_and_a_group_of_1025_are_refused(hip_lib):
    a = abi.DetectSoftNmsArgs()
    a.struct_size -= 8
    assert hip_lib.t3d_detect_soft_nms(C.byref(a), C.c_void_p(0)) == abi.ERR_ABI
    a = abi.DetectSoftNmsArgs(n=2000, n_groups=1, metric=0, max_group=1025, method=abi.SOFT_NMS_GAUSSIAN, sigma=0.5, min_score=0.001)
    assert hip_lib.t3d_detect_soft_nms(C.byref(a), C.c_void_p(0)) == -2


def test_soft_nms_beside_the_views_the_consistency_measures_and_the_pictures(rt, tmp_path):
    print('\n'.join(SC.check_stages(rt, tmp_path)))


def test_detect_with_soft_nms_equals_the_spec_on_the_plain_run_and_the_two_step_route(rt, tmp_path):
    print('\n'.join(SC.check_flow(rt, tmp_path, exact=False)))
