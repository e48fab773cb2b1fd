"""GPU: t3d_detect_ensemble (csrc/ensemble.hip) through ensemble.DeviceEnsemble against its NumPy fp64 specification
(tests/fake_ensemble.py) on the cases of tests/ensemble_check.py -- 1, 63, 64, 65 and 257 detections in 1, 2, 3, 5 and 8 views, mirrored
views, strays, quarter-turned writings of the same box, NaN labels, weights that count as 0, a case 45 m out, identical views, an outlying
view 0; both metrics at a vote threshold of 0 and of 0.5.  anchor, n_votes and which rows are byte copies are compared exactly, the numbers
within the bounds derived in ensemble_check (conditions on the inputs that test_detect_ensemble_cpu.py checks on the same seeds).  Then
the flow on the golden scenes through libt3d.so."""
import ctypes as C

import numpy as np
import pytest

import ensemble_check as EC
import fake_ensemble as FE
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.mark.parametrize('metric,vote', EC.PASSES)
def test_kernel_equals_the_spec(rt, metric, vote):
    for name in EC.cases(metric, vote):
        print(EC.check_case(rt, name, metric, vote))


def test_two_runs_give_equal_bytes(rt):
    for name in ('n65_v8', 'n257_v5', 'far_45m', 'non_finite'):
        c = EC.cases('3d', 0.5)[name]
        a, b = EC.run_case(rt, c, '3d', 0.5), EC.run_case(rt, c, '3d', 0.5)
        assert all(a[k].tobytes() == b[k].tobytes() for k in FE.OUTPUTS), name


@pytest.mark.parametrize('metric,vote', [('3d', 0.5), ('bev', 0.0)])
def test_the_same_detections_elsewhere_in_a_larger_call(rt, metric, vote):
    """Other row indices, other detections between them: per detection, the bytes of the call that holds the case alone."""
    for name in ('n65_v8', 'n64_v3', 'n63_v2', 'n1_v8', 'n64_v1'):
        got, alone = EC.moved(rt, name, metric, vote, seed=5), EC.run_case(rt, EC.cases(metric, vote)[name], metric, vote)
        assert all(got[k].tobytes() == alone[k].tobytes() for k in FE.OUTPUTS), name + ' moved'


def test_no_detection_nothing_written(rt):
    c = EC.cases('3d', 0.0)['n64_v3']
    got = EC.run(rt, c.labels[:, :0], c.weights[:, :0], np.zeros((0, 8, 3), np.float32), c.flip_mask, None, 0.0, '3d')
    assert all(len(got[k]) == 0 for k in FE.OUTPUTS)
    # the buffers of a larger run keep what they held when a call with n == 0 follows on them
    import torch
    from transferable3d_amd import ensemble as EN
    dev = EN.DeviceEnsemble(rt)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)
    out = dev.run([up(c.labels[v]) for v in range(c.V)], [up(c.weights[v]) for v in range(c.V)], up(c.corners0().reshape(-1, 24)), c.flip_mask,
                  up(c.rot), 0.0, '3d', fill=EC.FILL)
    for t, f in zip((dev.label, dev.corners, dev.agreement, dev.min_iou, dev.anchor, dev.n_votes), EC.FILL):
        t.fill_(f)
    dev._args.n = 0
    dev.relaunch()
    for t, f in zip((dev.label, dev.corners, dev.agreement, dev.min_iou, dev.anchor, dev.n_votes), EC.FILL):
        assert (t.cpu().numpy() == f).all()


def test_a_short_struct_nine_views_and_a_mirrored_view_0_are_refused(hip_lib):
    a = abi.DetectEnsembleArgs()
    a.struct_size -= 8
    assert hip_lib.t3d_detect_ensemble(C.byref(a), C.c_void_p(0)) == abi.ERR_ABI
    assert hip_lib.t3d_detect_ensemble(C.byref(abi.DetectEnsembleArgs(n=4, V=9, metric=0, vote_threshold=0.5)), C.c_void_p(0)) == -2
    assert hip_lib.t3d_detect_ensemble(C.byref(abi.DetectEnsembleArgs(n=4, V=3, metric=0, vote_threshold=0.5, flip_mask=0b011)), C.c_void_p(0)) == -1


def test_detect_with_views_equals_the_spec_on_its_own_view_labels(rt, tmp_path):
    """detect --tta 3 --tta_flip on the golden scenes; --tta 2 keeps view 0 byte-equal to the plain run."""
    print('\n'.join(EC.check_flow(rt, tmp_path, exact=False)[0]))
