"""GPU: t3d_scene_floor and t3d_detect_floor (csrc/floor.hip) through libt3d.so against the NumPy specification tests/fake_floor.py, as
bytes (tests/floor_check.py says why no tolerance exists), and the floor stage end to end on generated scenes."""
import numpy as np
import pytest

import floor_check as FC
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.mark.parametrize('ld', [3, 6])
@pytest.mark.parametrize('S', [1, 3, 9])
def test_scene_floor_equals_the_specification(rt, S, ld):
    """hist, counts and plane, byte for byte, for scenes of 0 .. 8193 points mixed in one call."""
    FC.check_batch(rt, S, ld)


def test_scene_floor_where_a_workgroup_walks_two_chunks(rt):
    FC.check_two_rounds(rt)


def test_scene_floor_constructed_cases(rt):
    """The lowest of two planes, a share just below and at min_share, heights on bin edges, a plateau, rows that are not finite, a tilt
    that is accepted, a strip and a tilt beyond the limit."""
    FC.check_constructed(rt)


def test_a_scenes_bytes_do_not_depend_on_its_batch(rt):
    FC.check_batch_independence(rt)


def test_refusals_come_before_any_launch(hip_lib):
    FC.check_scene_floor_refusals(hip_lib)
    FC.check_detect_floor_refusals(hip_lib)


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('n', FC.DETECT_SIZES)
def test_detect_floor_equals_the_specification(rt, n, mode):
    FC.check_detect_floor(rt, n, mode)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(hip_lib):
    """Four generated scenes through a plain Detector, one that measures and one that stretches, with the graph's initial weights."""
    import detect_check as DC
    import scene_check as SK
    from transferable3d_amd import detect as DT, test_semisup as TS
    rt = Runtime(lib=hip_lib)
    ss = SK.scene_set(rt, 4)
    scenes = [{'points': s['depth'], 'Rtilt': s['Rtilt'], 'K': s['K']} for s in ss.scenes]
    dets = [s['detections'] for s in ss.scenes]
    out = {'scenes': ss.scenes}
    for name, kw in (('plain', {}), ('floor', dict(floor=True, floor_min_share=0.02)), ('stretch', dict(snap_floor='stretch', snap_floor_max=100.0))):
        det = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, **kw)
        parts = [det.extract(scenes, dets, ss.ids)]
        out[name] = (det.detect(scenes, dets, scene_ids=ss.ids), parts)
    return out


def test_measuring_changes_no_box(runs):
    plain, floor = runs['plain'][0], runs['floor'][0]
    n = 0
    for a, b in zip(plain, floor):
        assert len(a) == len(b)
        for r, q in zip(a, b):
            assert FC.same(np.asarray(r['label']), np.asarray(q['label'])) and FC.same(np.asarray(r['corners']), np.asarray(q['corners']))
            assert r['score'] == q['score'] and 'floor_gap' in q and 'floor_gap' not in r and np.isfinite(q['floor_gap'])
            n += 1
    assert n >= 4


def test_stretching_stands_every_box_on_the_floor_and_keeps_its_top(runs):
    floor, stretch = runs['floor'][0], runs['stretch'][0]
    n = 0
    for a, b in zip(floor, stretch):
        for r, q in zip(a, b):
            assert q['floor_gap'] == r['floor_gap']                      # the gap is the one measured before snapping
            if not q['floor_flags'] & abi.DETECT_FLOOR_SNAPPED:
                assert FC.same(np.asarray(r['label']), np.asarray(q['label']))
                continue
            yf = r['floor_gap'] + r['label'][4]
            assert q['label'][4] == np.float32(yf)
            top0, top1 = r['label'][4] - r['label'][0], q['label'][4] - q['label'][0]
            assert abs(top1 - top0) <= 2.0 ** -23 * max(abs(top0), abs(yf), 1.0) * 2
            assert np.array_equal(np.asarray(q['corners'])[:, [0, 2]], np.asarray(r['corners'])[:, [0, 2]])
            n += 1
    assert n >= 4


def test_every_scenes_plane_lies_within_one_bin_of_its_room(runs):
    part = runs['floor'][1][0]
    plane, counts = part['floor']['plane'].cpu().numpy(), part['floor']['counts_host']
    for s, sc in enumerate(runs['scenes']):
        assert not counts[s, 3] & abi.FLOOR_NONE, (s, counts[s])
        a, b, c, mx, my = plane[s, :5]
        print('scene %d: floor %.4f, room %.4f, share %.2f' % (sc['id'], a * mx + b * my + c, sc['room'][4], counts[s, 1] / counts[s, 0]))
        assert abs((a * mx + b * my + c) - sc['room'][4]) <= 0.02
