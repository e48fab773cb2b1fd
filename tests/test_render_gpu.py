"""GPU: t3d_render (csrc/render.hip) through render.Renderer against its NumPy fp64 specification (tests/fake_render.py), byte for byte:
the shared cases of tests/render_check.py (two views of 64 x 48 and 33 x 17 per call; depth contests, ties, splats at the borders, every
kind of segment in both directions, thickness, far endpoints, the near plane, a NaN corner, the painting order, backgrounds, the gaps
of `out`), the three fixture scenes at 320 x 240 with image, points, label boxes and detection rectangles, Detector.detect(...,
vis_dir=...) and the viewer.  No tolerance on any picture: the cases keep every decision a margin away from its boundary (render_check's repair rule)."""
import ctypes as C

import numpy as np
import pytest

import fake_render as FR
import render_check as RC
from transferable3d_amd import abi, render as R
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.mark.parametrize('name', sorted(RC.cases()))
def test_kernel_equals_the_spec(rt, name):
    c = RC.cases()[name]
    got, want = RC.run_case(rt, c), RC.expected(name)
    print('%-20s %4d points %2d boxes %2d rectangles, %d redrawn: %d bytes differ' % (name, len(c.xyz), len(c.boxes), len(c.rects), c.redrawn,
                                                                                     int((got != want).sum())))
    RC.assert_equal(got, want, name)


def test_the_device_checks_its_entries_without_the_host_mirrors(rt):
    for name in ('random', 'near_plane', 'thickness'):
        RC.assert_equal(RC.run_case(rt, RC.cases()[name], mirrors=False), RC.expected(name), name)


def test_two_runs_give_equal_bytes(rt):
    ren = R.Renderer(rt)
    for name in ('random', 'planes', 'order'):
        a, b = RC.run_case(rt, RC.cases()[name], ren), RC.run_case(rt, RC.cases()[name], ren)
        assert a.tobytes() == b.tobytes(), name


def test_empty_call_and_errors(rt):
    assert R.Renderer(rt).render([]) == []
    for what, want, call in RC.error_calls(rt):
        assert call() == want, what


def test_hand_built_pictures(rt):
    seg = np.array([[2, 3, 1.0]] * 4 + [[7, 3, 1.0]] * 4, np.float32)[None]
    xyz = np.array([[5, 5, 3.0], [5, 5, 2.0], [8, 2, 1.0], [8, 2, 1.0]], np.float32)
    rgb = np.array([(1, 0, 0), (0, 0, 1), (1, 0, 0), (0, 0, 1)], np.float32)
    a, b = R.Renderer(rt).render([R.View(np.eye(4), 12, 16).boxes(seg, (1.0, 1.0, 1.0)), R.View(np.eye(4), 12, 16).points(xyz, rgb=rgb)])
    ys, xs = np.nonzero(a.any(2))
    assert sorted(zip(xs.tolist(), ys.tolist())) == [(x, 3) for x in range(2, 8)]
    assert tuple(b[5, 5]) == (0, 0, 255) and tuple(b[2, 8]) == (255, 0, 0) and int(b.any(2).sum()) == 2


@pytest.mark.parametrize('k', range(3))
def test_fixture_scenes_at_320_by_240(rt, k):
    """Image, points, label boxes and detection rectangles of a fixture scene: byte-equal to the specification, and every corner the
    reference's box3d_pts_2d puts inside the image carries its box's colour (unless a later primitive lies over it)."""
    c = RC.scene_case(k)
    got = RC.run_case(rt, c)
    RC.assert_equal(got, c.expected(), c.name)
    checked, covered = RC.check_reference_corners(c, k, got)
    print('%s: %d points, %d redrawn; %d reference corners inside the image, %d under a later primitive' % (c.name, len(c.xyz), c.redrawn, checked, covered))
    assert checked >= 8 and covered < checked / 2


def test_detect_with_vis_dir_writes_the_files_and_the_same_records(rt, tmp_path):
    import json
    import os
    import detect_check as DC
    from transferable3d_amd import detect as DT, test_semisup as TS
    ids, _, _, dets = DC.write_data_set(tmp_path)
    scenes = DC.load_scenes(tmp_path, ids)
    pictures = RC.scenes()[0]
    for s, p in zip(scenes, pictures):
        s.update(image=p['image'], gt_corners=p['gt'], gt_classes=p['gt_classes'])
    det = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt)              # the graph's initial weights
    plain = det.detect(scenes, dets, scene_ids=ids)
    vis_dir = str(tmp_path / 'pics')
    drawn = det.detect(scenes, dets, scene_ids=ids, vis_dir=vis_dir, vis_gt=True)
    assert len(plain) == len(drawn) and all(len(a) == len(b) for a, b in zip(plain, drawn))
    for a, b in zip(plain, drawn):
        for ra, rb in zip(a, b):
            assert ra['class'] == rb['class'] and ra['prob'] == rb['prob'] and ra['score'] == rb['score']
            assert all(np.array_equal(ra[key], rb[key]) for key in ('box2d', 'label', 'corners'))
    with_boxes = [s for s, recs in zip(ids, plain) if recs]
    assert with_boxes and sorted(os.listdir(vis_dir)) == sorted('%06d.%s' % (s, e) for s in with_boxes for e in ('png', 'json'))
    for s, recs in zip(ids, plain):
        if not recs:
            continue
        png = R.read_png(os.path.join(vis_dir, '%06d.png' % s))
        legend = json.load(open(os.path.join(vis_dir, '%06d.json' % s)))
        assert png.shape == (240, 320 + 4 + 240, 3)
        assert [b['class'] for b in legend['boxes'] if b['kind'] == 'kept'] == [r['class'] for r in recs]
        assert (png == FR.to_byte(R.GT_COLOUR)).all(2).any()              # the label boxes, in both panels
        assert (png[:, :320] == FR.to_byte(R.GT_COLOUR)).all(2).any() and (png[:, 324:] == FR.to_byte(R.GT_COLOUR)).all(2).any()


def test_viewer_pred3d_and_fpc_on_the_device(rt, tmp_path):
    """python -m transferable3d_amd.viewer through libt3d.so: t3d_box3d_iou_corners behind the `Mean Box IOU` line (held to 2e-5 of the
    fp64 specification, the bound tests/test_dataset_gpu.py holds the device IoU to), t3d_frustum_extract and t3d_render behind the pictures."""
    print('\n'.join(RC.check_viewer(rt, tmp_path, 2e-5)))
