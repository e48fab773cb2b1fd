"""GPU: the bootstrap over images through libt3d.so (csrc/sunrgbd_bootstrap.hip) on the cases of tests/bootstrap_check.py.  The weights
are compared byte for byte with the header's hash in Python integers.  The reference of every replicate's curve is the specification's
LITERAL expansion of the resampled data set, scored by the EXISTING kernel (t3d_sunrgbd_eval) -- never a weighted curve: the counts are
compared exactly and the AP within 1e-12 absolute.  The weighted area is a sum of at most P <= 3000 terms in [0, 1] in fp64 and the
literal one adds each block's steps one by one, so the two differ by reordering and regrouping alone, which 3000 * 2^-52 < 7e-13 bounds."""
import ctypes as C

import numpy as np
import pytest

import bootstrap_check as BC
import fake_bootstrap as FB
from transferable3d_amd import abi, bootstrap as BS, evaluate_sunrgbd as ES
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


# ---- t3d_bootstrap_weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_images,R', [(1, 1), (7, 3), (300, 65), (5000, 4)])
def test_weights_are_the_hash_of_the_header(rt, n_images, R):
    w = BS.Weights(rt, n_images, R, seed=3)
    got = w.numpy()
    assert got.dtype == np.int32 and got.shape == (R, n_images)
    assert got.tobytes() == FB.weights(3, R, n_images).tobytes()
    assert (got.sum(1) == n_images).all() and (got >= 0).all()
    assert BS.Weights(rt, n_images, R, seed=3).numpy().tobytes() == got.tobytes(), 'two calls differ'
    if n_images > 1:
        assert BS.Weights(rt, n_images, R, seed=4).numpy().tobytes() != got.tobytes(), 'the seed does not reach the draws'


def test_weights_leave_the_padding_columns_zero_and_refuse(rt, hip_lib):
    import torch
    m = torch.full((3, 12), 77, dtype=torch.int32, device=rt.device)
    a = abi.BootstrapWeightsArgs(9, 3, 7, 12, abi.iptr(m))
    assert hip_lib.t3d_bootstrap_weights(C.byref(a), rt.stream()) == 0
    got = m.cpu().numpy()
    assert got[:, :7].tobytes() == FB.weights(9, 3, 7).tobytes() and (got[:, 7:] == 0).all()
    for bad, rc in ((dict(R=0), -2), (dict(R=65537), -2), (dict(n_images=0), -2), (dict(stride=6), -1), (dict(weights=None), -1)):
        a = abi.BootstrapWeightsArgs(9, 3, 7, 12, abi.iptr(m))
        for k, v in bad.items():
            setattr(a, k, v)
        assert hip_lib.t3d_bootstrap_weights(C.byref(a), rt.stream()) == rc, bad
    a.struct_size -= 8
    assert hip_lib.t3d_bootstrap_weights(C.byref(a), rt.stream()) == abi.ERR_ABI
    assert m.cpu().numpy().tobytes() == got.tobytes(), 'a refused call wrote'


# ---- t3d_sunrgbd_eval_bootstrap -------------------------------------------------------------------------------------------------------
# EV_CURVE_THREADS = 1024: P = 1023, 1024, 1025 lie on both sides of one detection per thread, 63 / 64 / 65 of one wave, 3000 gives uneven
# chunks of 3.  Every G of {0, 1, 40} and every R of {1, 3, 65} occurs; R = 1 is the hand-made row (zeros, 1 .. 3, one large multiplicity),
# R >= 3 adds the rows of ones and of zeros, R = 65 rows drawn by the hash.  P <= 65: the large multiplicity is 1000.
@pytest.mark.parametrize('P,G,R', [(0, 0, 1), (0, 40, 3), (1, 1, 3), (1, 0, 1), (63, 40, 65), (64, 1, 3), (65, 40, 3), (1023, 40, 3), (1024, 1, 65),
                                   (1025, 40, 1), (3000, 40, 3), (3000, 1, 1), (3000, 0, 3)])
def test_replicates_equal_the_literal_expansion(rt, P, G, R):
    """Tied and NaN confidences across images, detections in images without ground truth, an image whose columns lie outside the matrix,
    zeros, a multiplicity of 1000, an all-zero row: n_pos, n_tp, n_fp exactly those of t3d_sunrgbd_eval on the literally resampled data
    set, ap within 1e-12; every output of the evaluation the bytes of a plain call; two calls equal bytes."""
    BC.check_curves(rt, P, G, R)


@pytest.mark.parametrize('P,G', [(0, 40), (1, 1), (63, 40), (64, 1), (65, 40), (1023, 40), (1024, 1), (1025, 40), (3000, 40), (3000, 0)])
def test_a_row_of_ones_is_the_evaluation_bit_for_bit(rt, P, G):
    BC.check_ones(rt, P, G)


def test_a_row_too_long_for_lds_is_gathered_with_the_same_bytes(rt):
    """weight_stride 70 000 is 280 KB, beyond any LDS: the global-gather path, against the same case at stride 300.  Stride 30 000 is
    120 KB: a row in LDS beyond the 64 KB a launch gets without asking."""
    det, gt = BC.case(1025, 40, seed=2)
    out = []
    for stride in (300, 30000, 70000):
        det_col, gt_col = BC.columns(det, gt, seed=2, stride=stride)
        w = BC.matrix(5, 7, seed=2, stride=stride)
        out.append(BC.run(rt, det, gt, w, det_col, gt_col))
    assert BC.same_bytes(out[0], out[1]) and BC.same_bytes(out[0], out[2])
    assert len(set(out[0]['boot']['ap'].tolist())) >= 3 and out[0]['boot']['n_tp'].max() > 0


# ---- evaluate --bootstrap -------------------------------------------------------------------------------------------------------------
def test_evaluate_with_bootstrap_equals_the_specification_on_the_golden_scenes(rt, tmp_path):
    import detect_check as DC
    ids, _, idx, _ = DC.write_data_set(tmp_path)
    held = BC.held_of(BC.golden_rows(tmp_path, ids, seed=1))
    got_lines, want_lines = [], []
    got = ES.evaluate(None, str(tmp_path), idx, 'AB', rt=rt, log=got_lines.append, predictions=held, bootstrap=128)
    want = ES.evaluate(None, str(tmp_path), idx, 'AB', rt=BC.spec_rt(), log=want_lines.append, predictions=held, bootstrap=128)
    assert got[2]['R'] == 128 and sorted(got[2]['ap']) == sorted(ES.CLASS_NAMES['AB'])
    for c in ES.CLASS_NAMES['AB']:
        assert got[2]['ap'][c].shape == (128,)
        assert np.abs(got[2]['ap'][c] - want[2]['ap'][c]).max() <= 1e-12, c
    assert got_lines == want_lines and sum(l.startswith('AP interval for ') for l in got_lines) == 10 and got_lines[-1].startswith('Mean AP interval: [')
    assert max(np.ptp(v) for v in got[2]['ap'].values()) > 0.0, 'no replicate differs from another'
