"""GPU: t3d_scene_range and t3d_detect_visibility (csrc/range.hip) through libt3d.so against the NumPy specification
tests/fake_visibility.py, as bytes (tests/visibility_check.py says why no tolerance exists), and the visibility stage end to end on
generated scenes."""
import numpy as np
import pytest

import visibility_check as VC
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.mark.parametrize('ld', [3, 6])
@pytest.mark.parametrize('S', [1, 3])
def test_scene_range_equals_the_specification(rt, S, ld):
    """The cells and the counts, byte for byte, for scenes of 0, 1, 255, 257 and 4097 points under three cameras."""
    VC.check_range_batch(rt, S, ld)


def test_scene_range_constructed_cases(rt):
    """Points on a cell border, at u = W, outside the image, behind the camera, not finite, two in one cell, the partial last cell."""
    VC.check_range_constructed(rt)


def test_scene_range_flags_a_scene_it_cannot_bin(rt):
    VC.check_range_flags(rt)


def test_a_scenes_cells_do_not_depend_on_its_batch(rt):
    VC.check_range_batch_independence(rt)


def test_refusals_come_before_any_launch(hip_lib):
    VC.check_scene_range_refusals(hip_lib)
    VC.check_detect_visibility_refusals(hip_lib)


def test_detect_visibility_counts_what_was_counted_by_hand(rt):
    """A box in front of a wall is seen through, one around it holds it, one behind it is occluded; a hole in the map is unknown."""
    VC.check_hand_cases(rt)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('K', [1, 3, 9])
@pytest.mark.parametrize('n', VC.DETECT_SIZES)
def test_detect_visibility_equals_the_specification(rt, n, K, mode):
    VC.check_detect_visibility(rt, n, K, mode)


def test_a_detections_bytes_do_not_depend_on_its_batch(rt):
    VC.check_detect_batch_independence(rt)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(hip_lib):
    """Four generated scenes through a plain Detector and one that measures, with the graph's initial weights."""
    import detect_check as DC
    import scene_check as SK
    from transferable3d_amd import detect as DT, test_semisup as TS
    rt = Runtime(lib=hip_lib)
    ss = SK.scene_set(rt, 4)
    scenes = [{'points': s['depth'], 'Rtilt': s['Rtilt'], 'K': s['K']} for s in ss.scenes]
    dets = [s['detections'] for s in ss.scenes]
    out = {'scenes': ss.scenes}
    for name, kw in (('plain', {}), ('measure', dict(visibility=True))):
        det = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, **kw)
        parts = [det.extract(scenes, dets, ss.ids)]
        meta, d = det.decode_all(parts)
        out[name] = (det.detect(scenes, dets, scene_ids=ss.ids), parts, meta, d, det)
    return out


def test_measuring_changes_no_box_and_a_run_without_the_flags_is_the_unchanged_path(runs):
    plain, measure = runs['plain'][0], runs['measure'][0]
    n = 0
    for a, b in zip(plain, measure):
        assert len(a) == len(b)
        for r, q in zip(a, b):
            assert list(q)[:len(r)] == list(r) and list(q)[len(r):] == ['see_through', 'occluded', 'support', 'visibility_flags']
            assert all(np.asarray(r[k]).tobytes() == np.asarray(q[k]).tobytes() for k in r)
            assert 0.0 <= q['see_through'] <= 1.0
            n += 1
    assert n >= 4
    d = runs['plain'][3]
    assert d.see_through is None and d.visibility_flags is None and 'range' not in runs['plain'][1][0]


def test_the_records_equal_the_specification_on_the_same_boxes_and_map(runs):
    import fake_visibility as FV
    _, parts, meta, d, det = runs['measure']
    part, o = parts[0]['range'], det.visibility.options
    rng = part['range'].cpu().numpy().view(np.uint32)
    points = np.concatenate([s['depth'] for s in runs['scenes']])
    offsets = np.concatenate([[0], np.cumsum([len(s['depth']) for s in runs['scenes']])])
    want_rng, want_counts = FV.scene_range_batch(points, offsets, part['calib'], np.arange(4), part['dims'], part['offsets'], len(rng), o.cell)
    assert VC.same(rng, want_rng) and VC.same(part['counts'], want_counts) and (want_counts[:, 2] > 20).all()
    want = FV.detect_visibility(d.label.astype(np.float32), d.corners.astype(np.float32), [m.scene for m in meta], part['calib'], part['dims'],
                                part['offsets'], rng, o.cell, [0.0], o.margin, o.min_chord, 0, 0)
    assert np.array_equal(d.visibility_profile, want[0][:, 0]) and VC.same(np.stack([d.see_through, d.occluded, d.support], 1), want[1])
    assert np.array_equal(d.visibility_flags, want[3]) and (d.visibility_profile[:, 0] > 0).any()
