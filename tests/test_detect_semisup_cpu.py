"""CPU: semisup_infer --device_decode on the specification library, synthetic frustums and a frustum file: the same detections as the
host decode, --evaluate and --official_eval read the decoded records, the pickled 14-list keeps its layout."""
import pickle
import gzip

import numpy as np

import sunrgbd_eval_check as K
from fake_detect import DetectDecodeSpec
from fake_sunrgbd_eval import FakeSunrgbdEvalLib
from transferable3d_amd import semisup_infer as TS
from transferable3d_amd.engine import Runtime


class SpecLib(DetectDecodeSpec, FakeSunrgbdEvalLib):
    pass


ARGV = ['--semi_type', 'F', '--use_one_hot', '--num_point', '128', '--num_channels', '4', '--batch_size', '4', '--refine', '1',
        '--pred_prefix', 'F2_', '--synthetic', '--num_frustums', '6', '--evaluate']


def test_synthetic_run_with_device_decode_equals_the_host_decode(tmp_path):
    logs = {}
    out = {}
    for tag, extra in (('host', []), ('device', ['--device_decode'])):
        logs[tag] = []
        path = str(tmp_path / (tag + '.pickle'))
        out[tag] = TS.test(TS.build_flags(ARGV + ['--output', path] + extra), rt=Runtime(device='cpu', lib=SpecLib()), log=logs[tag].append)
        with gzip.open(path, 'rb') as f:
            back = pickle.load(f)
        assert type(back) is list and len(back) == 14
    h, d = out['host'], out['device']
    assert h.decoded is None and len(d.decoded) == 8 and d.decoded.corners.shape == (8, 8, 3)
    for k in (2, 4, 6):                                       # masks and classes
        assert np.array_equal(np.asarray(h[k]), np.asarray(d[k])), k
    for k in (3, 5, 7, 9):                                    # fp32 stores of the fp64 specification against the fp64 host decode
        assert np.abs(np.asarray(h[k], np.float64) - np.asarray(d[k], np.float64)).max() <= 1e-6, k
    ap = lambda lines: [l for l in lines if 'Average Precision' in str(l)]
    assert ap(logs['host']) and ap(logs['host']) == ap(logs['device'])


def test_official_eval_passes_the_flag_through(tmp_path, monkeypatch):
    """evaluate_sunrgbd --official_eval ... --device_decode: the lines equal those of evaluate() on the files the same run wrote."""
    seen = []
    real = TS.build_flags
    monkeypatch.setattr(TS, 'build_flags', lambda argv=None: seen.append(real(argv)) or seen[-1])
    import transferable3d_amd.evaluate_sunrgbd as ES
    main = ES.main
    monkeypatch.setattr(ES, 'main', lambda argv, **kw: main(list(argv) + ['--device_decode'], **kw))
    lines = K.check_test_semisup_official_eval(Runtime(device='cpu', lib=SpecLib()), tmp_path, num_point=128)
    assert len(lines) == 21 and seen and seen[-1].device_decode
