"""CPU: the NumPy specification of t3d_detect_decode (tests/fake_detect.py) against the reference's recorded post-processing
(tests/golden/reference_vectors.npz: infer/*, p2l/*, results/*), and semisup_infer.inference(decode='device') on it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import detect_check as DC
import fake_detect as FD
from transferable3d_amd import abi
from transferable3d_amd import constants as K
from transferable3d_amd import eval_det as E
from transferable3d_amd import semisup_infer as TS
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH, NS = K.NUM_HEADING_BIN, K.NUM_SIZE_CLUSTER


@pytest.fixture(scope='module')
def V():
    return DC.golden_vectors()


def test_spec_reproduces_the_recorded_inference_outputs(V):
    logits, box, s1, fit = DC.golden_net(V)
    for tag, f in (('plain', None), ('with_fit', fit)):
        r = FD.decode(logits, box, s1, None, f, None)
        for nm in ('seg', 'center', 'heading_cls', 'heading_res', 'size_cls', 'size_res', 'score'):
            want = V['infer/%s/%s' % (tag, nm)]
            assert r[nm].shape == want.shape and np.abs(r[nm] - want).max() <= 1e-12, (tag, nm)
    assert r['mask_count'][5] == 0 and not V['infer/plain/seg'][5].any()      # the empty mask: the "+ 1" denominator alone
    assert abs(r['score'][5] - V['infer/with_fit/score'][5]) <= 1e-12


def test_spec_reproduces_the_recorded_label_format_rows(V):
    n = len(V['p2l/out'])
    box = np.zeros((n, FD.BOX))
    r = np.arange(n)
    box[:, 0:3] = V['p2l/center']
    box[r, 3 + V['p2l/angle_cls']] = 1.0
    box[r, 3 + NH + V['p2l/angle_cls']] = V['p2l/angle_res'] / (np.pi / NH)
    box[r, 3 + 2 * NH + V['p2l/size_cls']] = 1.0
    for b in range(n):
        k = int(V['p2l/size_cls'][b])
        box[b, 3 + 2 * NH + NS + 3 * k:3 + 2 * NH + NS + 3 * k + 3] = V['p2l/size_res'][b] / K.MEAN_DIMS_ARR[k]
    out = FD.decode(np.zeros((n, 4, 2)), box, np.zeros((n, 3)), None, None, V['p2l/rot'])
    assert np.array_equal(out['heading_cls'], V['p2l/angle_cls']) and np.array_equal(out['size_cls'], V['p2l/size_cls'])
    assert np.abs(out['label'] - V['p2l/out']).max() <= 1e-12
    assert np.abs(V['p2l/rot']).max() > 0.1


def test_spec_corners_are_get_3d_box_of_its_own_label(V):
    for c in DC.cases().values():
        r = DC.spec(c)
        for b in range(len(r['label'])):
            h, w, l, tx, ty, tz, ry = r['label'][b]
            assert np.abs(r['corners'][b] - E.get_3d_box((l, w, h), ry, (tx, ty - h / 2, tz))).max() <= 1e-12
    for s, h, c, want in zip(V['box/size'], V['box/heading'], V['box/center'], V['box/corners']):
        assert np.abs(FD.get_3d_box(s[0], s[1], s[2], h, c) - want).max() <= 1e-12


class _T:
    """What semisup_infer.decode_sources reads of an api.Tensor."""

    def __init__(self, buf, name=None, src=None):
        self.buf, self.name, self.src = buf, name, src


@pytest.mark.parametrize('wide', [True, False])
def test_inference_with_device_decode_writes_the_reference_result_files(V, tmp_path, wide):
    """The prepared-array session of test_inference_post_processing_and_result_files, its arrays lying in the buffers the decode reads.
    wide: fp64 buffers end to end (FakeDetectLib(wide=True)) -- the files equal the reference's as text.  Through the fp32 ABI an output
    below 8 is stored within 2^-22 / 2 = 2.4e-7 of the fp64 value, which can turn over the sixth decimal of a printed number: there every
    number is within one unit of the last printed digit (1e-6, compared with 1.5e-6 for the parse) and everything else is equal.
    The files are not written from what inference returned: this session feeds arrays and has no rotation angles, while results/file/*
    were recorded with results/rot, so the label rows come from a second call of the specification with those angles (only `center` ties
    the two together).  The chain inference -> Decoded.label -> writer with non-zero rotation is covered by the scene-flow tests
    (tests/test_detect_cpu.py, tests/test_detect_gpu.py)."""
    logits, box, s1, fit = DC.golden_net(V)
    tot, bsz = len(box), 4
    rt = (DC.WideRuntime if wide else Runtime)(device='cpu', lib=FD.FakeDetectLib(wide=wide))
    dt = torch.float64 if wide else torch.float32
    buf = {k: torch.zeros(shape, dtype=dt) for k, shape in (('logits', (bsz, 32, 2)), ('box', (bsz, FD.BOX)), ('s1', (bsz, 3)), ('fit', (bsz,)))}
    box_t = _T(buf['box'], 'F_box_params')
    head = lambda: _T(None, src=box_t)
    ops = {'pc_pl': 'pc', 'one_hot_vec_pl': 'oh', 'logits': _T(buf['logits']),
           'end_points': {'F_center': head(), 'F_heading_scores': head(), 'stage1_center': _T(buf['s1']), 'boxpc_fit_prob': _T(buf['fit'])}}

    class Session:
        class g:
            pass

        def __init__(self):
            self.i = 0
            self.g.rt = rt

        def run(self, run_ops, feed_dict=None):
            assert run_ops == []                                  # nothing is fetched between the graph and the decode
            sl = slice(self.i * bsz, (self.i + 1) * bsz)
            self.i += 1
            for k, a in (('logits', logits), ('box', box), ('s1', s1), ('fit', fit)):
                buf[k].copy_(torch.as_tensor(a[sl]).to(dt))
            return []
    pcs, ohs = np.zeros((tot, 32, 4)), np.zeros((tot, 10))
    for tag, use_fit in (('plain', False), ('with_fit', True)):
        res = TS.inference(Session(), ops, pcs, ohs, bsz, prefix='F_', use_boxpc_fit_prob=use_fit, decode='device')
        assert len(res) == 7 and len(res.decoded) == tot
        for nm, v in zip(('seg', 'center', 'heading_cls', 'heading_res', 'size_cls', 'size_res', 'score'), res):
            want = V['infer/%s/%s' % (tag, nm)]
            assert np.asarray(v).shape == want.shape and np.allclose(v, want, atol=1e-12 if wide else 2e-6), (tag, nm)
        if tag == 'plain':
            plain = res
    names = [str(t) for t in V['results/type']]
    # the label rows of these files were computed with rot_angle = results/rot: decode them again with it (the session above has none)
    d = FD.decode(logits, box, s1, None, None, V['results/rot'])
    if not wide:
        d = {k: v.astype(np.float32).astype(np.float64) if v.dtype == np.float64 else v for k, v in d.items()}
    assert np.abs(d['center'] - plain.decoded.center).max() <= (0 if wide else 1e-6)
    predictions = TS.Predictions([None, None, None, list(plain[1]), list(plain[2]), list(plain[3]), list(plain[4]), list(plain[5]),
                                  list(V['results/rot']), list(V['infer/plain/score']), None, list(V['results/ids']), list(V['results/box2d']), None])
    predictions.decoded = TS.Decoded(**{k: d[k] for k in TS.Decoded.FIELDS})
    classes = [str(c) for c in V['results/classes']]
    TS.write_detection_results(str(tmp_path / 'res'), classes, predictions, names)
    for c in classes:
        got, want = (tmp_path / 'res' / (c + '_pred.txt')).read_text(), str(V['results/file/' + c])
        if wide:
            assert got == want, c
        else:
            for x, y in zip(got.splitlines(), want.splitlines()):
                x, y = x.split(), y.split()
                assert x[:9] == y[:9] and x[16] == y[16] and max(abs(float(p) - float(q)) for p, q in zip(x[9:16], y[9:16])) <= 1.5e-6
            assert len(got.splitlines()) == len(want.splitlines())


def test_decode_argument_is_checked():
    with pytest.raises(ValueError):
        TS.inference(None, None, np.zeros((4, 8, 4)), None, 4, decode='gpu')


def test_ctypes_struct_follows_the_header(tmp_path):
    from test_sunrgbd_extract_cpu import _header_fields
    assert _header_fields('t3d_detect_decode_args') == [f[0] for f in abi.DetectDecodeArgs._fields_]
    src = tmp_path / 's.c'
    src.write_text('#include <stdio.h>\n#include "t3d.h"\nint main(void){printf("%zu %d\\n", sizeof(t3d_detect_decode_args), '
                   'T3D_V2_SIZE_detect_decode_args);return 0;}\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 's')])
    size, v2 = [int(v) for v in subprocess.check_output([str(tmp_path / 's')], text=True).split()]
    assert size == v2 == C.sizeof(abi.DetectDecodeArgs) and abi.DetectDecodeArgs().struct_size == size
    assert abi.ENTRY_POINTS['t3d_detect_decode'][0]._type_ is abi.DetectDecodeArgs


def test_the_library_refuses_bad_arguments_without_a_launch():
    lib = abi.load()
    null = C.c_void_p(0)
    a = abi.DetectDecodeArgs()
    a.struct_size -= 8
    assert lib.t3d_detect_decode(C.byref(a), null) == abi.ERR_ABI
    assert lib.t3d_detect_decode(C.byref(abi.DetectDecodeArgs()), null) == -2          # B = 0
    a = abi.DetectDecodeArgs(4, 32, 4, 67)
    assert lib.t3d_detect_decode(C.byref(a), null) == -1                               # null pointers
    a.ld_box = 66
    assert lib.t3d_detect_decode(C.byref(a), null) == -2
    fake = FD.FakeDetectLib()
    assert fake.t3d_detect_decode(C.byref(abi.DetectDecodeArgs(4, 32, 4, 67)), null) == -1
    assert fake.t3d_detect_decode(C.byref(abi.DetectDecodeArgs()), null) == -2
