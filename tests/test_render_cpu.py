"""CPU: the headless rasteriser (t3d_render, transferable3d_amd/render.py, detect --vis_dir, python -m transferable3d_amd.viewer) on
the NumPy specification (tests/fake_render.py): hand-built pictures whose answer needs no projection code, the shared cases, the
argument struct, the view builders against the reference's own projections, write_png, and the two user-facing routes end to end."""
import ctypes as C
import json
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import fake_render as FR
import render_check as RC
from fake_frustum import FakeFrustumLib
from transferable3d_amd import abi, render as R
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SpecLib(FR.RenderSpec, FR.DetectNmsSpec, FR.DetectDecodeSpec, FakeFrustumLib):
    pass


def cpu_rt():
    return Runtime(device='cpu', lib=SpecLib())


# ---- hand-built answers ----------------------------------------------------------------------------------------------------------------
WHITE, RED, BLUE = (1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)


def lit(img):
    """The painted pixels of a picture on a black background, as a sorted list of (x, y)."""
    ys, xs = np.nonzero(img.any(2))
    return sorted(zip(xs.tolist(), ys.tolist()))


def one_view(H=12, W=16):
    return R.View(np.eye(4), H, W, w_near=0.5)          # u = x, v = y, D = z, W = 1


def segment_box(a, b):
    return np.array([[a[0], a[1], 1.0]] * 4 + [[b[0], b[1], 1.0]] * 4, np.float32)[None]


def test_a_horizontal_segment_paints_exactly_its_six_pixels():
    v = one_view().boxes(segment_box((2, 3), (7, 3)), WHITE)
    img, = R.Renderer(cpu_rt()).render([v])
    assert img.shape == (12, 16, 3) and img.dtype == np.uint8
    assert lit(img) == [(x, 3) for x in range(2, 8)] and (img[3, 2:8] == 255).all()


def test_the_two_to_one_slope():
    """(1,1) -> (9,5): the minor coordinate is 1 + floor((2 (m - 1) 4 + 8) / 16) = 1 + floor((m - 1) / 2 + 1 / 2): a half rounds up."""
    want = [(1, 1), (2, 2), (3, 2), (4, 3), (5, 3), (6, 4), (7, 4), (8, 5), (9, 5)]
    for a, b in (((1, 1), (9, 5)), ((9, 5), (1, 1))):
        img, = R.Renderer(cpu_rt()).render([one_view().boxes(segment_box(a, b), WHITE)])
        assert lit(img) == want
    assert FR.segment_pixels(1, 1, 9, 5) == want == sorted(FR.segment_pixels(9, 5, 1, 1))
    # steep, upwards: the same rule with the axes exchanged
    assert sorted(FR.segment_pixels(5, 9, 1, 1)) == sorted((y, x) for x, y in want)
    assert FR.segment_pixels(4, 4, 4, 4) == [(4, 4)]
    # thickness 2 stamps offsets 0 .. +1, thickness 3 offsets -1 .. +1
    img, = R.Renderer(cpu_rt()).render([one_view().boxes(segment_box((4, 4), (4, 4)), WHITE, thickness=2)])
    assert lit(img) == [(4, 4), (4, 5), (5, 4), (5, 5)]
    img, = R.Renderer(cpu_rt()).render([one_view().boxes(segment_box((0, 0), (0, 0)), WHITE, thickness=3)])
    assert lit(img) == [(0, 0), (0, 1), (1, 0), (1, 1)]                        # clipped to the view


def test_the_nearer_of_two_points_wins_and_an_equal_depth_goes_to_the_lower_index():
    xyz = np.array([[5, 5, 3.0], [5, 5, 2.0], [8, 2, 1.0], [8, 2, 1.0]], np.float32)
    rgb = np.array([RED, BLUE, RED, BLUE], np.float32)
    img, = R.Renderer(cpu_rt()).render([one_view().points(xyz, rgb=rgb)])
    assert lit(img) == [(5, 5), (8, 2)]
    assert tuple(img[5, 5]) == (0, 0, 255) and tuple(img[2, 8]) == (255, 0, 0)
    # pixel centres sit on integers: 4.49 is pixel 4, 4.51 is pixel 5; a point behind w_near or with D < 0 is not painted
    xyz = np.array([[4.49, 1, 1.0], [4.51, 2, 1.0], [7, 7, -1.0]], np.float32)
    img, = R.Renderer(cpu_rt()).render([one_view().points(xyz)])
    assert lit(img) == [(4, 1), (5, 2)]
    # splat 3 at a corner, boxes over points, rectangles over boxes
    v = one_view().points(np.array([[0, 0, 1.0]], np.float32), splat=3, colour0=RED)
    v.boxes(segment_box((0, 0), (3, 0)), BLUE).rects([(1, 0, 1, 0)], WHITE)
    img, = R.Renderer(cpu_rt()).render([v])
    assert lit(img) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (3, 0)]
    assert tuple(img[0, 0]) == (0, 0, 255) and tuple(img[0, 1]) == (255, 255, 255) and tuple(img[1, 1]) == (255, 0, 0)


def test_colour_conversion():
    assert FR.to_byte([0.0, 1.0, -3.0, 7.0, np.nan, 0.25, 127.4 / 255]).tolist() == [0, 255, 0, 255, 0, 64, 127]
    for c in R.CLASS_PALETTE + (R.GT_COLOUR, R.SUPPRESSED_COLOUR, R.POINT_COLOUR) + R.MASK_COLOURS:
        v = FR.colour_value(c)
        assert (np.abs(v - np.round(v)) > 0.4).all(), c                       # b / 255 * 255 + 0.5: half-way between two boundaries
    assert len(R.CLASS_PALETTE) == 10 and len(set(R.CLASS_PALETTE)) == 10


# ---- the shared cases ------------------------------------------------------------------------------------------------------------------
def test_generated_cases_keep_the_margins():
    for name, c in RC.cases().items():
        assert c.redrawn <= RC.MAX_REDRAWN * c.n_primitives, name
        assert c.bad_primitives() == (set(), set(), set()), name
        assert len(c.xyz) <= 2000 and len(c.boxes) <= 12 and [(v['H'], v['W']) for v in c.views] == list(RC.SIZES)
        assert sum(b['view'] == 0 for b in c.boxes) <= 6 and sum(b['view'] == 1 for b in c.boxes) <= 6


def test_what_the_cases_are_there_for():
    cs = RC.cases()
    img = lambda name, i=0: RC.view_image(cs[name], RC.expected(name), i)
    # B -> A paints what A -> B paints
    for n in ('segments_a', 'segments_b'):
        for i in range(2):
            assert (img(n, i) == img(n + '_reversed', i)).all() and img(n, i).any()
    # the box behind the near plane and the one with a NaN corner paint nothing; the crossing one does
    c = cs['near_plane']
    colours = lambda i: set(map(tuple, img('near_plane', i).reshape(-1, 3).tolist()))
    for i in range(2):
        assert tuple(FR.to_byte(RC.colour_of(3)).tolist()) in colours(i)
        assert tuple(FR.to_byte(RC.colour_of(4)).tolist()) not in colours(i) and tuple(FR.to_byte(RC.colour_of(5)).tolist()) not in colours(i)
    # a view with no primitives shows its background colour, the other its image where nothing was painted
    c = cs['background']
    assert (img('background', 1) == np.array([200, 100, 255], np.uint8)).all()
    same = (img('background', 0) == c.views[0]['image']).all(2)
    assert 0.5 < same.mean() < 1.0
    # the tie: index 0 wins pixel (5, 5) of the first view and is coloured by its own range; in the second view the later range comes first
    assert tuple(img('tie')[5, 5]) == tuple(FR.to_byte(RC.colour_of(1)).tolist())
    assert tuple(img('tie', 1)[5, 5]) == tuple(FR.to_byte(RC.colour_of(4)).tolist())
    # painting order: the crossing of the two thick segments belongs to the later one; the rectangles lie over everything
    o = img('order')
    top = lambda x, y: tuple(o[y, x].tolist())
    assert top(20, 10) == tuple(FR.to_byte(RC.colour_of(5)).tolist()) and top(25, 20) == tuple(FR.to_byte(RC.colour_of(6)).tolist())
    assert top(32, 22) in (tuple(FR.to_byte(RC.colour_of(3)).tolist()), tuple(FR.to_byte(RC.colour_of(4)).tolist()))
    # the gaps of every case keep the fill pattern
    for name, c in cs.items():
        buf, (offs, n, _, _) = RC.expected(name), c.layout()
        fill = RC.fill_pattern(n)
        gap = np.ones(n, bool)
        for o_, v in zip(offs, c.views):
            gap[o_:o_ + 3 * v['H'] * v['W']] = False
        assert gap.sum() == sum(RC.GAPS) and (buf[gap] == fill[gap]).all(), name


def test_renderer_on_the_specification_library():
    rt = cpu_rt()
    ren = R.Renderer(rt)
    for name, c in RC.cases().items():
        RC.assert_equal(RC.run_case(rt, c, ren), RC.expected(name), name)
    a, b = RC.run_case(rt, RC.cases()['random']), RC.run_case(rt, RC.cases()['random'], mirrors=False)
    assert a.tobytes() == b.tobytes()


def test_empty_call_and_errors():
    rt = cpu_rt()
    assert R.Renderer(rt).render([]) == []
    for lib_rt in (rt, Runtime(device='cpu', lib=abi.load())):          # the specification and the built library: the checks come before any launch
        for what, want, call in RC.error_calls(lib_rt):
            assert call() == want, (what, type(lib_rt.lib).__name__)


# ---- the argument struct ---------------------------------------------------------------------------------------------------------------
def test_structs_follow_the_header_and_the_compiler(tmp_path):
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    pairs = {'t3d_render_args': abi.RenderArgs, 't3d_render_view': abi.RenderView, 't3d_render_points': abi.RenderPoints,
             't3d_render_box': abi.RenderBox, 't3d_render_rect': abi.RenderRect}
    for cname, cls in pairs.items():
        body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\}\s*%s;' % cname, h).group(1), flags=re.S)
        names = [re.findall(r'(\w+)(?:\[\d+\])?\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]
        assert names == [f[0] for f in cls._fields_], cname
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include "t3d.h"\nint main(void) { printf("%zu %d %zu %zu %zu %zu %llu %d %d %d\\n", sizeof(t3d_render_args), '
                   'T3D_V2_SIZE_render_args, sizeof(t3d_render_view), sizeof(t3d_render_points), sizeof(t3d_render_box), sizeof(t3d_render_rect), '
                   '(unsigned long long)T3D_RENDER_WORKSPACE_BYTES(730 * 530 * 16), T3D_RENDER_RGB, T3D_RENDER_LABEL, T3D_RENDER_FLAT); return 0; }\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'size')])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / 'size')], text=True).split()]
    assert got[0] == got[1] == C.sizeof(abi.RenderArgs) and abi.RenderArgs().struct_size == got[0]
    assert got[2:6] == [C.sizeof(x) for x in (abi.RenderView, abi.RenderPoints, abi.RenderBox, abi.RenderRect)]
    assert got[6] == abi.render_workspace_bytes(730 * 530 * 16) == 12 * 730 * 530 * 16
    assert got[7:] == [abi.RENDER_RGB, abi.RENDER_LABEL, abi.RENDER_FLAT] == [FR.RGB, FR.LABEL, FR.FLAT]


# ---- the view builders against the reference's own projections -------------------------------------------------------------------------
def test_image_view_projects_as_the_reference_does():
    """render.image_view (its fp64 matrix) composed with the specification's transform against utils.compute_box_3d's box3d_pts_2d and
    SUNRGBD_Calibration.project_upright_depth_to_image, recorded by tests/golden/make_render_vectors.py: 1e-6 px."""
    from transferable3d_amd import sunrgbd_data as SD
    scenes, ref = RC.scenes()
    assert [s['id'] for s in scenes] == ref['ids'].tolist()
    worst = 0.0
    for s in scenes:
        v = R.image_view(s['Rtilt'], s['K'], *RC.SCENE_SIZE)
        P = v.P                                                       # fp64: the rounding to fp32 is the device's, bounded in render_check
        def uv_of(cam):
            h = np.concatenate([cam, np.ones((len(cam), 1))], 1) @ P.T
            assert np.allclose(h[:, 2], h[:, 3])                      # D = W = the camera depth
            return h[:, :2] / h[:, 3:4], h[:, 2]
        k3 = ref['box_depth_corners_%d' % s['id']]
        assert ref['box_class_%d' % s['id']].tolist() == s['gt_classes']
        for j in range(len(k3)):
            assert np.abs(SD.flip_axis_to_camera(k3[j]) - s['gt'][j]).max() < 1e-12          # the label code's corners are the reference's
            uv, _ = uv_of(s['gt'][j])
            worst = max(worst, np.abs(uv - ref['box_uv_%d' % s['id']][j]).max())
        pick = ref['point_index_%d' % s['id']]
        uv, depth = uv_of(s['xyz'][pick])
        worst = max(worst, np.abs(uv - ref['point_uv_%d' % s['id']]).max(), np.abs(depth - ref['point_depth_%d' % s['id']]).max())
    print('image_view against the reference: worst %.3g px' % worst)
    assert worst < 1e-6


def test_orthographic_builders():
    img, = R.Renderer(cpu_rt()).render([R.bev_view((-2.0, 2.0), (0.0, 8.0), 8, 4).points(
        np.array([[-1.9, 0.0, 0.1], [1.9, 0.0, 7.9], [0.1, 1.0, 4.1], [0.1, -1.0, 4.1]], np.float32),
        rgb=np.array([WHITE, WHITE, RED, BLUE], np.float32))])
    assert lit(img) == [(0, 7), (2, 3), (3, 0)]                       # near-left at the bottom-left, far-right at the top-right
    assert tuple(img[3, 2]) == (0, 0, 255)                            # y points down: the higher point (y = -1) hides the lower
    img, = R.Renderer(cpu_rt()).render([R.side_view((0.0, 8.0), (-2.0, 2.0), 4, 8).points(
        np.array([[0.0, -1.9, 0.1], [0.0, 1.9, 7.9], [1.0, 0.1, 4.1], [-1.0, 0.1, 4.1]], np.float32),
        rgb=np.array([WHITE, WHITE, RED, BLUE], np.float32))])
    assert lit(img) == [(0, 0), (4, 2), (7, 3)] and tuple(img[2, 4]) == (0, 0, 255)      # up at the top; the nearer x wins
    (x0, x1), (y0, y1), (z0, z1) = R.ranges_of(np.array([[0, 0, 1.0], [2, 1, 2.0], [np.nan, 0, 0]]))
    assert x0 < 0 < 2 < x1 and y0 < 0 < 1 < y1 and abs((x1 - x0) - (z1 - z0)) < 1e-12


# ---- write_png -------------------------------------------------------------------------------------------------------------------------
def test_write_png_round_trips(tmp_path):
    r = np.random.RandomState(0)
    for shape in ((17, 33, 3), (1, 1, 3), (5, 4)):
        a = r.randint(0, 256, shape).astype(np.uint8)
        path = str(tmp_path / ('a%d.png' % len(shape)))
        R.write_png(path, a)
        assert (R.read_png(path) == a).all()
        try:
            from PIL import Image
        except ImportError:
            data = open(path, 'rb').read()                             # no imaging package: inflate the one IDAT chunk by hand
            at = data.index(b'IDAT')
            n = int.from_bytes(data[at - 4:at], 'big')
            rows = np.frombuffer(zlib.decompress(data[at + 4:at + 4 + n]), np.uint8).reshape(shape[0], -1)
            assert not rows[:, 0].any() and (rows[:, 1:].reshape(shape) == a).all()
        else:
            with Image.open(path) as im:
                assert (np.asarray(im) == a).all()
    with pytest.raises(ValueError):
        R.write_png(str(tmp_path / 'bad.png'), np.zeros((2, 2, 4), np.uint8))
    tiles = [np.full((4, 6, 3), k, np.uint8) for k in range(5)]
    assert R.side_by_side([tiles[0], np.zeros((7, 3, 3), np.uint8)], gap=1).shape == (7, 6 + 1 + 3, 3)


# ---- detect --vis_dir ------------------------------------------------------------------------------------------------------------------
def test_detect_vis_dir_writes_panels_and_legends_and_changes_nothing_else(tmp_path):
    import detect_check as DC
    import nms_check as NC
    from transferable3d_amd import detect as DT, test_semisup as TS
    rt, quiet = cpu_rt(), (lambda *a: None)
    ids, folder, idx, dets = NC.write_duplicated(tmp_path)
    base = ['--dataset_dir', str(tmp_path), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS
    res = lambda name: os.path.join(str(tmp_path), name)
    # without the new flags: the parent's outputs (detect_check's and nms_check's own flows compare those with the two-step route)
    DT.main(base + ['--result_dir', res('plain')], rt=rt, log=quiet)
    DT.main(base + ['--result_dir', res('plain_nms'), '--nms_iou', str(NC.FLOW_T)], rt=rt, log=quiet)
    logged = []
    DT.main(base + ['--result_dir', res('vis'), '--vis_dir', res('pics')], rt=rt, log=logged.append)
    assert DC.read_results(res('vis')) == DC.read_results(res('plain'))
    assert any('%d scenes drawn' % len(ids) in l for l in logged), logged
    DT.main(base + ['--result_dir', res('vis_nms'), '--nms_iou', str(NC.FLOW_T), '--vis_dir', res('pics_nms'), '--vis_gt', '--vis_suppressed',
                    '--vis_max', '2'], rt=rt, log=quiet)
    assert DC.read_results(res('vis_nms')) == DC.read_results(res('plain_nms'))
    assert sorted(os.listdir(res('pics'))) == sorted('%06d.%s' % (s, e) for s in ids for e in ('png', 'json'))
    assert sorted(os.listdir(res('pics_nms'))) == sorted('%06d.%s' % (s, e) for s in ids[:2] for e in ('png', 'json'))
    scenes = DC.load_scenes(tmp_path, ids)
    plain = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt).detect(scenes, dets, scene_ids=ids)
    kept = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, nms_iou=NC.FLOW_T).detect(scenes, dets, scene_ids=ids)
    for k, s in enumerate(ids):
        png = R.read_png(os.path.join(res('pics'), '%06d.png' % s))
        assert png.shape == (240, 320 + 4 + 240, 3)                              # the camera panel, a gap, the square bird's-eye panel
        legend = json.load(open(os.path.join(res('pics'), '%06d.json' % s)))
        assert legend['scene'] == s and legend['panels'] == {'image': [240, 320], 'bev': [240, 240]}
        boxes = legend['boxes']
        assert [b['class'] for b in boxes] == [r['class'] for r in plain[k]] and all(b['kept'] and b['kind'] == 'kept' for b in boxes)
        assert np.allclose([b['score'] for b in boxes], [r['score'] for r in plain[k]]) and np.allclose([b['prob'] for b in boxes], [r['prob'] for r in plain[k]])
        assert all(b['colour'] == FR.to_byte(R.class_colour(b['class'])).tolist() for b in boxes)
        # a box colour is in both panels, and the camera panel still shows the image somewhere
        for b in boxes:
            for panel in (png[:, :320], png[:, 324:]):
                assert (panel == np.array(b['colour'], np.uint8)).all(2).any(), (s, b['class'])
        if k < 2:
            legend = json.load(open(os.path.join(res('pics_nms'), '%06d.json' % s)))
            by_kind = lambda kind: [b for b in legend['boxes'] if b['kind'] == kind]
            assert len(by_kind('gt')) == len(RC.scenes()[0][k]['gt_classes']) and [b['class'] for b in by_kind('gt')] == RC.scenes()[0][k]['gt_classes']
            assert [b['class'] for b in by_kind('kept')] == [r['class'] for r in kept[k]]
            assert len(by_kind('suppressed')) == len(plain[k]) - len(kept[k]) > 0
            kept_ids = {b['detection'] for b in by_kind('kept')}
            assert all(not b['kept'] and b['suppressed_by'] in kept_ids and b['colour'] == FR.to_byte(R.SUPPRESSED_COLOUR).tolist() for b in by_kind('suppressed'))
            png = R.read_png(os.path.join(res('pics_nms'), '%06d.png' % s))
            for c in (R.GT_COLOUR, R.SUPPRESSED_COLOUR):
                assert (png == FR.to_byte(c)).all(2).any()
    # Detector.detect with the keyword arguments: the same records, the same files
    again = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt).detect(scenes, dets, scene_ids=ids, vis_dir=res('pics_api'), vis_max=1)
    assert DC.record_lines(ids, again) == DC.record_lines(ids, plain)
    assert sorted(os.listdir(res('pics_api'))) == ['%06d.json' % ids[0], '%06d.png' % ids[0]]
    K = scenes[0]['K']                                         # no image given: twice the principal point, and the points are drawn
    h, w = int(2 * K[1, 2] + 0.5), int(2 * K[0, 2] + 0.5)
    png = R.read_png(os.path.join(res('pics_api'), '%06d.png' % ids[0]))
    assert png.shape == (h, w + 4 + h, 3) and (png[:, :w] != 0).any(2).mean() > 0.02
    needed = ['--dataset_dir', str(tmp_path), '--idx_path', idx, '--rgb_detection_path', folder]
    for extra in (['--vis_gt'], ['--vis_suppressed'], ['--vis_dir', res('x'), '--vis_suppressed'], ['--vis_dir', res('x'), '--vis_max', '-1']):
        with pytest.raises(SystemExit):
            DT.main(needed + extra, rt=rt, log=quiet)
    with pytest.raises(ValueError):
        DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt).detect(scenes, dets, scene_ids=ids, vis_dir=res('y'), vis_suppressed=True)


# ---- python -m transferable3d_amd.viewer -----------------------------------------------------------------------------------------------
def test_viewer_pred3d_and_fpc_end_to_end(tmp_path):
    """The specification library's box IoU is fp64 arithmetic stored as fp32: 2^-24 per box."""
    print('\n'.join(RC.check_viewer(cpu_rt(), tmp_path, 2.0 ** -24)))


def test_get_seg_iou_by_hand():
    from transferable3d_amd import viewer as VW
    assert VW.get_seg_iou([1, 1, 0, 0], [1, 0, 0, 0]) == 0.5 * (1 / 2.0 + 2 / 3.0)
    assert VW.get_seg_iou([1, 0], [1, 0]) == 1.0 and VW.get_seg_iou([1, 1], [0, 0]) == 0.0
    assert VW.get_seg_iou([0, 0], [0, 0]) == 1.0                  # no foreground in either: that class counts 1
    k = np.arange(24, dtype=np.float64).reshape(8, 3)
    assert (VW.y_max_face_first(k) == k[[4, 5, 6, 7, 0, 1, 2, 3]]).all() and (VW.y_max_face_first(k[::-1]) == k[::-1]).all()
    assert np.allclose(VW.rotate_along_y(np.array([[1.0, 5.0, 0.0]]), np.pi / 2), [[0.0, 5.0, 1.0]])
