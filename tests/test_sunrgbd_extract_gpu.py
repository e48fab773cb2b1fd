"""GPU: frustum extraction through libt3d.so (t3d_frustum_extract) -- the golden comparison of tests/test_sunrgbd_extract_cpu.py on the
reference's own draws, the generated draws (distinct, in range, independent of the batch, keyed by seed and augmentation index, uniform
inclusion), a full-size scene against tests/ref_frustum.py, and the ABI size check.  The entry point itself at its edges (ragged batches,
the cut at num_points, hash ties, exact boundaries, guard bands): tests/test_kernels_frustum_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import frustum_check as FC
from fake_frustum import FakeFrustumLib
from transferable3d_amd import abi
from transferable3d_amd import sunrgbd_data as SD
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture
def rt(hip_lib):
    return Runtime(lib=hip_lib)


def test_golden_roi_seg_on_the_reference_draws(rt, tmp_path):
    ids, det, z = FC.write_golden_scenes(tmp_path)
    lists = SD.extract_roi_seg(str(tmp_path), ids, augmentX=int(z['augmentX']), perturb_box2d=True, rt=rt, draws=FC.golden_draws(z))
    FC.check_roi_seg(lists, tmp_path, ids)


def test_golden_detections_on_the_reference_draws(rt, tmp_path):
    ids, det, z = FC.write_golden_scenes(tmp_path)
    lists = SD.extract_roi_seg_from_rgb_detection(det, str(tmp_path), rt=rt, draws=FC.golden_draws(z, det=True))
    FC.check_detection(lists, tmp_path, ids)


def _scenes(rng, n_scenes, n_points=6000, n_boxes=4):
    scenes, jobs = [], []
    for s in range(n_scenes):
        depth, rtilt, K, boxes = FC.synthetic_scene(rng, n_points=n_points, n_boxes=n_boxes)
        # one wide box so that every scene subsamples
        boxes.append((np.array([100.37, 80.37, 650.37, 470.37]), boxes[0][1]))
        scenes.append({'points': depth, 'Rtilt': rtilt, 'K': K})
        for k, (box, corners) in enumerate(boxes):
            jobs.append({'scene': s, 'box2d': box, 'box3d': corners, 'key': (100 + s, k, 0)})
    return scenes, jobs


def _run(rt_, scenes, jobs, seed=0, per_scene=False, perturb=True):
    ex = SD.FrustumExtractor(rt_, 512, seed=seed)
    if not per_scene:
        return ex.run(scenes, jobs, perturb_box2d=perturb)
    out = []
    for s in range(len(scenes)):
        js = [dict(j, scene=0) for j in jobs if j['scene'] == s]
        out += ex.run([scenes[s]], js, perturb_box2d=perturb)
    return out


def _same(a, b, angle_tol=0.0):
    """bit-identical outputs (angle_tol: the frustum angle to within it -- the specification library's atan2 is not the device's)"""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x['n'] == y['n'] and np.array_equal(x['index'], y['index']), i
        assert np.array_equal(x['points'], y['points']) and np.array_equal(x['label'], y['label']), i
        assert np.array_equal(x['box2d'], y['box2d']), (i, x['box2d'], y['box2d'])
        assert abs(x['frustum_angle'] - y['frustum_angle']) <= angle_tol, (i, x['frustum_angle'], y['frustum_angle'])
    return True


def test_generated_draws_distinct_in_range_and_independent_of_the_batch(rt):
    scenes, jobs = _scenes(np.random.RandomState(4), 5)
    one = _run(rt, scenes, jobs)
    assert sum(r['n'] > 512 for r in one) >= 5
    for r in one:
        k = min(r['n'], 512)
        assert len(r['index']) == k and len(np.unique(r['index'])) == k and (r['index'] >= 0).all()
    assert _same(one, _run(rt, scenes, jobs))                      # two runs
    assert _same(one, _run(rt, scenes, jobs, per_scene=True))      # every scene in one launch / one scene per launch
    # the specification library draws the same
    assert _same(one, _run(Runtime(device='cpu', lib=FakeFrustumLib()), scenes, jobs), angle_tol=1e-12)
    other_seed = _run(rt, scenes, jobs, seed=1)
    other_aug = _run(rt, scenes, [dict(j, key=(j['key'][0], j['key'][1], 1)) for j in jobs])
    for a, b, c in zip(one, other_seed, other_aug):
        if a['n'] > 512:
            assert not np.array_equal(a['index'], b['index']) and not np.array_equal(a['index'], c['index'])


def test_inclusion_frequency_is_uniform(rt):
    """One scene, one box, M jobs (different ordinals) with n frustum points each: every rank is kept with probability k/n.  Bound: 6
    standard deviations of a binomial(M, k/n) frequency, fixed here; the specification library meets it."""
    rng = np.random.RandomState(9)
    depth, rtilt, K, _ = FC.synthetic_scene(rng, n_points=20000, n_boxes=1)
    box = np.array([200.37, 150.37, 420.37, 330.37])
    M, k = 400, 512
    jobs = [{'scene': 0, 'box2d': box, 'box3d': None, 'key': (7, m, 0)} for m in range(M)]
    out = SD.FrustumExtractor(rt, k, seed=11).run([{'points': depth, 'Rtilt': rtilt, 'K': K}], jobs)
    n = out[0]['n']
    assert n > 2 * k
    members = np.sort(np.unique(np.concatenate([r['index'] for r in out])))
    freq = np.zeros(depth.shape[0])
    for r in out:
        freq[r['index']] += 1.0 / M
    p = k / n
    bound = 6 * np.sqrt(p * (1 - p) / M)
    dev = np.abs(freq[members] - p).max()
    print('inclusion frequency: n %d, p %.4f, max deviation %.4f, bound %.4f' % (n, p, dev, bound))
    assert len(members) == n and dev <= bound          # every frustum point is drawn, none too often or too rarely


@pytest.mark.parametrize('detection', [False, True])
def test_full_size_scene_matches_the_restatement(rt, detection):
    FC.check_full_size(rt, np.random.RandomState(21 + int(detection)), detection)


def test_a_short_struct_is_refused(hip_lib):
    a = abi.FrustumExtractArgs()
    a.struct_size -= 8
    assert hip_lib.t3d_frustum_extract(C.byref(a), C.c_void_p(0)) == abi.ERR_ABI
