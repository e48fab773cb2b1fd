"""GPU: t3d_detect_consistency (csrc/consistency.hip) against its NumPy fp64 specification (tests/fake_consistency.py), bit for bit, and
what is built on it: Detector.detect(consistency=True), the filter in front of NMS, autolabel end to end.

Exactness.  The kernel and the specification perform the same IEEE fp64 operations in the same order, so with rot_angle NULL every
output is compared as bytes.  With rot_angle the projection outputs are still exact (the corners are in the camera frame already); the
counts are exact under the input condition consistency_check.case establishes and run_kernel asserts on the CPU before every launch: no
point lies closer than 1e-9 (relative to the edge) to a face, so a last-place difference between the device's and NumPy's cos / sin
cannot flip a point.  No case is left out for it: points are redrawn, the share of excluded cases is 0."""
import ctypes as C

import numpy as np
import pytest
import torch

import consistency_check as CC
import detect_check as DC
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


def same_bytes(got, want, what):
    for g, w, name in zip(got, want, ('counts', 'reproj')):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, g, w)


@pytest.mark.parametrize('with_rot', [False, True])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 255, 256, 257, 2048])
def test_kernel_equals_the_spec_bit_for_bit(rt, N, with_rot):
    for B, ld in ((1, 3), (3, 4), (32, 6)) if N in (65, 257, 2048) else ((3, 3 + N % 3 if N % 3 != 2 else 6),):
        c = CC.case(1000 + N + B, B, N, ld, with_rot)
        want = CC.spec(c)
        same_bytes(CC.run_kernel(rt, c), want, (N, B, ld))
        if B >= 3:                  # the cases the issue names are all here
            flags = want[0][:, 3]
            assert ((flags & 4) != 0).sum() == 1 and (flags & 2).any() and (want[0][:, 0] == N).any()
        if B == 32:
            assert (flags & 1).any() and (want[1][:, 4] == 1.0).any() and ((want[1][:, 4] > 0) & (want[1][:, 4] < 1)).any()
            assert ((want[0][:, 2] > 0) & (want[0][:, 2] < want[0][:, 1])).any()


@pytest.mark.parametrize('B', [1, 3, 32])
def test_rows_at_or_past_n_valid_keep_a_sentinel(rt, B):
    c = CC.case(77 + B, B, 65, 4, True)
    for n_valid in sorted({0, 1, B - 1, B}):
        got = CC.run_kernel(rt, c, n_valid=n_valid, sentinel=-77)
        same_bytes(got, CC.spec(c, n_valid=n_valid, sentinel=-77), (B, n_valid))
        assert (got[0][n_valid:] == -77).all() and (got[1][n_valid:] == -77.0).all()


def test_inclusive_faces_on_the_device(rt):
    c, inside = CC.faces_case()
    counts, _ = CC.run_kernel(rt, c)
    mask = c['logits'][0, :, 1] > c['logits'][0, :, 0]
    assert list(counts[0][:3]) == [mask.sum(), inside.sum(), (mask & inside).sum()]
    same_bytes((counts, _), CC.spec(c), 'faces')


def test_equal_bytes_whatever_the_batch_is(rt):
    for with_rot in (False, True):
        c = CC.case(5, 3, 257, 4, with_rot)
        a = CC.run_kernel(rt, c)
        same_bytes(CC.run_kernel(rt, c), a, 'again')
        same_bytes(CC.run_kernel(rt, c, pad=5), a, 'pad')


def test_n_mask_equals_the_decodes_mask_count(rt):
    for B, N in ((5, 65), (3, 2048)):
        c = CC.case(9, B, N, 3, True)
        d = {k: np.ascontiguousarray(v, np.float32) for k, v in DC.random_case(3, B, N).items()}
        d['logits'] = c['logits']
        dec, _ = DC.run_decode(rt, d)
        counts, _ = CC.run_kernel(rt, c)
        assert np.array_equal(counts[:, 0], dec.mask_count)


def test_error_codes_before_any_launch(rt, hip_lib):
    B, N = 2, 8
    dev = rt.device
    t = dict(xyz=torch.zeros(B * N * 3 + 1, device=dev), logits=torch.zeros(B * N * 2 + 2, device=dev), corners=torch.zeros(B * 24, device=dev),
             rot=torch.zeros(B, device=dev), box2d=torch.zeros(B * 4, dtype=torch.float64, device=dev),
             index=torch.zeros(B, dtype=torch.int32, device=dev), calib=torch.zeros(20, dtype=torch.float64, device=dev),
             counts=torch.full((B * 4,), -5, dtype=torch.int32, device=dev), reproj=torch.full((B * 5,), -5.0, dtype=torch.float64, device=dev))

    def call(**kw):
        v = dict(B=B, N=N, n_valid=B, ld_xyz=3, n_calib=1, null=None, logits_off=0)
        v.update(kw)
        p = {k: None if k == v['null'] else x for k, x in t.items()}
        lg = None if p['logits'] is None else p['logits'][v['logits_off']:]
        a = abi.DetectConsistencyArgs(v['B'], v['N'], v['n_valid'], v['ld_xyz'], abi.fptr(p['xyz']), abi.fptr(lg), abi.fptr(p['corners']),
                                      abi.fptr(p['rot']), abi.dptr(p['box2d']), abi.iptr(p['index']), abi.dptr(p['calib']), v['n_calib'],
                                      abi.iptr(p['counts']), abi.dptr(p['reproj']))
        return hip_lib.t3d_detect_consistency(C.byref(a), rt.stream())

    SHAPE, ARG = -2, -1
    for kw in (dict(B=0), dict(B=-1), dict(N=0), dict(n_valid=-1), dict(ld_xyz=2), dict(n_calib=-1)):
        assert call(**kw) == SHAPE, kw
    for name in ('xyz', 'logits', 'corners', 'box2d', 'index', 'calib', 'counts', 'reproj'):
        assert call(null=name) == ARG, name
    assert call(logits_off=1) == ARG                      # 4-byte aligned only
    assert hip_lib.t3d_detect_consistency(None, rt.stream()) == ARG
    short = abi.DetectConsistencyArgs()
    short.struct_size -= 8
    assert hip_lib.t3d_detect_consistency(C.byref(short), rt.stream()) == abi.ERR_ABI
    assert call(n_valid=0) == 0
    torch.cuda.synchronize()
    assert (t['counts'] == -5).all() and (t['reproj'] == -5.0).all()          # nothing was launched by any of them
    assert call(null='rot') == 0                          # rot_angle may be NULL
    torch.cuda.synchronize()
    assert (t['counts'] != -5).all()


# ---- scene level: the golden scenes of tests/golden/frustum_scenes.npz, the graph's initial weights ---------------------------------
def test_detector_measures_equal_the_spec_on_what_the_device_held(rt, tmp_path):
    CC.check_detector(rt, tmp_path)


def test_a_rejected_box_does_not_suppress_a_good_one(rt, tmp_path):
    print(CC.check_filter_before_nms(rt, tmp_path))


def test_autolabel_end_to_end(rt, tmp_path):
    s, threshold = CC.check_autolabel(rt, tmp_path)
    print({c: dict(v) for c, v in s['classes'].items()}, threshold)
