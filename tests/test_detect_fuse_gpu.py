"""GPU: t3d_detect_fuse (csrc/fuse.hip) through nms.DeviceNms + nms.DeviceFuse against its NumPy fp64 specification (tests/fake_fuse.py)
on the cases of tests/fuse_check.py -- nms_check's groups of 1, 2, 63, 64, 65, 130, 260 and 1024 boxes, 40 mixed groups with empty ones and
unlisted boxes, ties, NaN and -inf weights, the chain, identical and zero-volume boxes; both metrics at T = 0.25 and 0.5 with the vote
threshold at T, and one pass that votes above 0.6 over T = 0.25.  n_votes and which boxes are byte copies are compared exactly, the fused
numbers within the bound derived in fuse_check (no IoU near a threshold, no heading near a tie of the quarter turns: conditions
test_detect_fuse_cpu.py checks on the same seeds).  Then the flow on the duplicated golden scenes through libt3d.so."""
import ctypes as C

import numpy as np
import pytest

import fuse_check as FC
import nms_check as NC
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu

MOVED = ('mixed_40', 'size_65', 'chain', 'ties_nan', 'size_2', 'zero_volume', 'size_130', 'identical', 'size_1')


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.mark.parametrize('metric,threshold,vote', FC.PASSES)
def test_kernel_equals_the_spec(rt, metric, threshold, vote):
    for name in FC.cases(metric, threshold, vote):
        print(FC.check_case(rt, name, metric, threshold, vote))


@pytest.mark.parametrize('metric,threshold', [('3d', 0.25), ('bev', 0.5)])
def test_a_group_of_1024(rt, metric, threshold):
    assert [len(g) for g in FC.big_case(metric, threshold).groups] == [abi.DETECT_NMS_MAX_GROUP]
    print(FC.check_case(rt, 'group_1024', metric, threshold, threshold))


def test_two_runs_give_equal_bytes(rt):
    for name in ('mixed_40', 'size_130', 'size_260', 'ties_nan'):
        c = FC.cases('3d', 0.25, 0.25)[name]
        a, b = FC.run_case(rt, c, 0.25)[1], FC.run_case(rt, c, 0.25)[1]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name


@pytest.mark.parametrize('metric,threshold', [('3d', 0.5), ('bev', 0.25)])
def test_the_same_groups_elsewhere_in_a_larger_call(rt, metric, threshold):
    """Other box indices (interleaved with other groups' boxes and with unlisted ones), the groups in reversed order: per box, the bytes
    of the call that holds the case alone."""
    names = [k for k in MOVED if k in FC.cases(metric, threshold, threshold)]
    assert len(names) >= 8
    for name, got in zip(names, FC.moved(rt, names, metric, threshold, threshold, seed=3)):
        alone = FC.run_case(rt, FC.cases(metric, threshold, threshold)[name], threshold)[1]
        assert all(g.tobytes() == a.tobytes() for g, a in zip(got, alone)), name + ' moved'


def test_unlisted_boxes_keep_what_they_held(rt):
    c = FC.cases('3d', 0.25, 0.25)['mixed_40']
    _, (lo, ko, nv) = FC.run_case(rt, c, 0.25)
    u = np.asarray(c.unlisted)
    assert len(u) >= 4 and (lo[u] == FC.FILL[0]).all() and (ko[u] == FC.FILL[1]).all() and (nv[u] == FC.FILL[2]).all()
    listed = np.setdiff1d(np.arange(c.n), u)
    assert (nv[listed] >= -1).all() and (lo[listed] != FC.FILL[0]).all()
    k = np.stack([NC.corners_of(NC.unit_cube(0.0))] * 3)
    l = np.stack([FC.label_of(NC.unit_cube(0.0))] * 3)
    for offsets in ([0], [0, 0, 0]):                            # no group; empty groups only: nothing is launched, nothing written
        _, got = FC.run(rt, l, k, np.ones(3, np.float32), offsets, [], 0.25, '3d', 0.25)
        assert all((g == f).all() for g, f in zip(got, FC.FILL))


def test_a_short_struct_and_a_group_of_1025_are_refused(hip_lib):
    a = abi.DetectFuseArgs()
    a.struct_size -= 8
    assert hip_lib.t3d_detect_fuse(C.byref(a), C.c_void_p(0)) == abi.ERR_ABI
    a = abi.DetectFuseArgs(n=2000, n_groups=1, metric=0, max_group=1025, vote_threshold=0.5)
    assert hip_lib.t3d_detect_fuse(C.byref(a), C.c_void_p(0)) == -2


def test_detect_with_fusion_equals_the_spec_on_the_plain_run_and_the_two_step_route(rt, tmp_path):
    print('\n'.join(FC.check_flow(rt, tmp_path, exact=False)))
