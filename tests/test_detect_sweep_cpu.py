"""CPU: the threshold sweep (t3d_detect_nms_sweep, t3d_sunrgbd_eval_sweep, nms.DeviceNmsSweep, evaluate_sunrgbd.sweep, sweep.py, detect
--sweep) on the specification library (tests/fake_sweep.py): the argument structs, every refusal of the built library and of the
specification, hand cases whose answers need no code, the grid's order and tie rule, the flags, and the whole flow on the duplicated
golden scenes against one separate detect run per grid row."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fake_consistency as FK
import fake_nms as FN
import fake_sweep as FS
import nms_check as NC
import sunrgbd_eval_check as SC
import sweep_check as SW
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from fake_sunrgbd_eval import FakeSunrgbdEvalLib
from transferable3d_amd import abi, detect as DT, evaluate_sunrgbd as ES, sweep as SWP
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SpecLib(FS.SweepSpec, FK.ConsistencySpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib, FakeSunrgbdEvalLib):
    pass


def cpu_rt():
    return Runtime(device='cpu', lib=SpecLib())


# ---- the argument structs ------------------------------------------------------------------------------------------------------------
def header_fields(name):
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\}\s*%s;' % name, h).group(1), flags=re.S)
    return [re.findall(r'(\w+)(?:\[\d+\])?\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]


def test_structs_follow_the_header_and_the_compiler(tmp_path):
    assert 't3d_detect_nms_sweep' in abi.ENTRY_POINTS and 't3d_sunrgbd_eval_sweep' in abi.ENTRY_POINTS
    assert header_fields('t3d_detect_nms_sweep_args') == [f[0] for f in abi.DetectNmsSweepArgs._fields_]
    assert header_fields('t3d_sunrgbd_sweep_args') == [f[0] for f in abi.SunrgbdSweepArgs._fields_]
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "t3d.h"\nint main(void) { printf("%zu %d %zu %d %llu %llu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(t3d_detect_nms_sweep_args), T3D_V2_SIZE_detect_nms_sweep_args, sizeof(t3d_sunrgbd_sweep_args), '
                   'T3D_V2_SIZE_sunrgbd_sweep_args, (unsigned long long)T3D_DETECT_NMS_SWEEP_WORKSPACE_BYTES(1001, 130, 4), '
                   '(unsigned long long)T3D_SUNRGBD_SWEEP_WORKSPACE_BYTES(33, 40), offsetof(t3d_detect_nms_sweep_args, thresholds), '
                   'offsetof(t3d_detect_nms_sweep_args, config_threshold), offsetof(t3d_detect_nms_sweep_args, n_kept), '
                   'offsetof(t3d_sunrgbd_sweep_args, workspace), T3D_NMS_SWEEP_MAX_THRESHOLDS, T3D_SWEEP_MAX_CONFIGS); return 0; }\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'size')])
    v = [int(x) for x in subprocess.check_output([str(tmp_path / 'size')], text=True).split()]
    assert v[0] == v[1] == C.sizeof(abi.DetectNmsSweepArgs) == abi.DetectNmsSweepArgs().struct_size
    assert v[2] == v[3] == C.sizeof(abi.SunrgbdSweepArgs) == abi.SunrgbdSweepArgs().struct_size
    assert v[4] == abi.detect_nms_sweep_workspace_bytes(1001, 130, 4) == 4008 + 1001 * 3 * 4 * 8
    assert v[5] == abi.sunrgbd_sweep_workspace_bytes(33, 40) == 33 * 40 * 4 + 8
    assert v[6] == abi.DetectNmsSweepArgs.thresholds.offset and v[7] == abi.DetectNmsSweepArgs.config_threshold.offset
    assert v[8] == abi.DetectNmsSweepArgs.n_kept.offset and v[9] == abi.SunrgbdSweepArgs.workspace.offset
    assert (v[10], v[11]) == (abi.NMS_SWEEP_MAX_THRESHOLDS, abi.SWEEP_MAX_CONFIGS) == (FS.MAX_THRESHOLDS, FS.MAX_CONFIGS) == (16, 65536)


def nms_args(buf, **kw):
    f, i, u = C.cast(buf, abi.F), C.cast(buf, abi.I), C.cast(buf, abi.U8)
    a = abi.DetectNmsSweepArgs(n=10, n_groups=1, metric=0, corners=f, score=f, group_offsets=i, members=i, max_group=10, n_thresholds=2, M=3,
                               listed_stride=16, keep_stride=16, config_threshold=i, listed=u, workspace=C.addressof(buf),
                               workspace_bytes=abi.detect_nms_sweep_workspace_bytes(10, 10, 2), keep=u, n_kept=i)
    a.thresholds[0], a.thresholds[1] = 0.25, 0.5
    for k, v in kw.items():
        if k == 'threshold1':
            a.thresholds[1] = v
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize('which', ['built', 'specification'])
def test_the_suppression_checks_before_it_launches(which):
    """No GPU needed: everything below is refused before anything is launched -- by the built library and, with the same answers, by
    the specification library."""
    lib, null = (abi.load() if which == 'built' else SpecLib()), C.c_void_p(0)
    call = lambda a: lib.t3d_detect_nms_sweep(C.byref(a), null)
    a = abi.DetectNmsSweepArgs()
    a.struct_size -= 8
    assert call(a) == abi.ERR_ABI
    buf = (C.c_uint64 * 256)()
    for bad in (dict(max_group=1025), dict(M=0), dict(M=65537), dict(M=-1), dict(n_thresholds=0), dict(n_thresholds=17)):
        assert call(nms_args(buf, **bad)) == -2, bad                        # T3D_ERR_SHAPE
    for bad in (dict(metric=2), dict(metric=-1), dict(n=-1), dict(n_groups=-1), dict(max_group=-1), dict(threshold1=float('nan')),
                dict(workspace_bytes=abi.detect_nms_sweep_workspace_bytes(10, 10, 2) - 8), dict(workspace=C.addressof(buf) + 4),
                dict(keep_stride=9), dict(listed_stride=9)):
        assert call(nms_args(buf, **bad)) == -1, bad                        # T3D_ERR_ARG
    for k in ('corners', 'score', 'group_offsets', 'members', 'config_threshold', 'workspace', 'keep', 'n_kept'):
        assert call(nms_args(buf, **{k: None})) == -1, k
    assert call(abi.DetectNmsSweepArgs(M=1, n_thresholds=1)) == -1          # an empty call still has to say n_kept = 0 somewhere


def eval_args_pair(buf, P=4, G=2, **kw):
    d, i, u = C.cast(buf, abi.D), C.cast(buf, abi.I), C.cast(buf, abi.U8)
    a = abi.SunrgbdEvalArgs(P=P, G=G, det_centroid=d, det_basis=d, det_coeffs=d, det_confidence=d, det_image=i, gt_centroid=d, gt_basis=d, gt_coeffs=d,
                            gt_image=i, n_images=1, image_ids=i, image_gt_offsets=i, image_gt=i, threshold=0.25, workspace=C.addressof(buf),
                            workspace_bytes=abi.sunrgbd_eval_workspace_bytes(P, G), order=i, max_overlap=d, gt_idx=i, is_tp=u, is_fp=u, gt_assignment=i,
                            is_missed=u, precision=d, recall=d, ap=d)
    s = abi.SunrgbdSweepArgs(M=3, mask=u, det_index=None, mask_stride=8, workspace=C.addressof(buf),
                             workspace_bytes=abi.sunrgbd_sweep_workspace_bytes(3, G), ap=d, n_det=i, n_tp=i, n_fp=i)
    for k, v in kw.items():
        setattr(a if k in ('gt_difficult', 'ap_eval') else s, 'ap' if k == 'ap_eval' else k, v)
    return a, s


@pytest.mark.parametrize('which', ['built', 'specification'])
def test_the_evaluation_sweep_checks_before_it_launches(which):
    lib, null = (abi.load() if which == 'built' else SpecLib()), C.c_void_p(0)
    call = lambda a, s: lib.t3d_sunrgbd_eval_sweep(C.byref(a), C.byref(s), null)
    buf = (C.c_uint64 * 512)()
    a, s = eval_args_pair(buf)
    s.struct_size -= 8
    assert call(a, s) == abi.ERR_ABI
    a, s = eval_args_pair(buf)
    a.struct_size -= 8
    assert call(a, s) == abi.ERR_ABI
    for bad in (dict(M=0), dict(M=65537)):
        assert call(*eval_args_pair(buf, **bad)) == -2, bad
    for bad in (dict(ap=None), dict(n_det=None), dict(n_tp=None), dict(n_fp=None), dict(mask=None), dict(mask_stride=3), dict(workspace=None),
                dict(workspace_bytes=abi.sunrgbd_sweep_workspace_bytes(3, 2) - 8), dict(workspace=C.addressof(buf) + 4),
                dict(gt_difficult=C.cast(buf, abi.U8)), dict(ap_eval=None)):
        assert call(*eval_args_pair(buf, **bad)) == -1, bad


# ---- hand cases: the suppression ------------------------------------------------------------------------------------------------------
def hand(boxes, scores, groups, thresholds, ct, listed=None, metric='3d', rt=None):
    corners = np.stack([NC.corners_of(b) for b in boxes])
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    members = np.asarray([b for g in groups for b in g], np.int32)
    listed = None if listed is None else np.asarray(listed, np.uint8)
    keep, n_kept = SW.run_nms_sweep(rt or cpu_rt(), corners, np.asarray(scores, np.float32), offsets, members, thresholds, ct, listed, metric)
    assert list(n_kept) == list(keep.sum(1))
    return [list(r) for r in keep]


CHAIN = [NC.unit_cube(0.0), NC.unit_cube(0.25), NC.unit_cube(0.5)]        # A covers B (IoU 3/5), B covers C, A and C overlap by 1/3


def test_chain_and_a_box_listed_in_one_configuration_only():
    """A > B > C.  Above 0.5: A suppresses B, and C, which only B would have suppressed, stays.  Above 0.25 A suppresses both.  Without B
    nothing changes for C; without A, B is kept and suppresses C.  Without a threshold every listed box stays."""
    keep = hand(CHAIN, [0.9, 0.8, 0.7], [[0, 1, 2]], [0.5, 0.25], [0, 1, 0, 0, -1, -1, 1],
                [[1, 1, 1], [1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0, 1, 0], [0, 0, 1]])
    assert keep == [[1, 0, 1], [1, 0, 0], [1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 1, 0], [0, 0, 1]]
    assert hand(CHAIN, [0.9, 0.8, 0.7], [[0, 1, 2]], [0.5], [0, -1]) == [[1, 0, 1], [1, 1, 1]]       # listed NULL: every box


def test_an_empty_row_a_box_in_no_group_and_an_index_that_names_no_threshold():
    boxes = CHAIN + [NC.unit_cube(9.0)]
    keep = hand(boxes, [0.9, 0.8, 0.7, 0.6], [[0, 1, 2]], [0.5], [0, -1, 0, 1, -2], [[0, 0, 0, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]])
    assert keep == [[0, 0, 0, 0], [1, 1, 1, 0], [1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]


def test_nan_scores_and_zero_volume_pairs():
    """A NaN score ranks as -inf (behind every real score; equal keys by box index).  Two boxes without extent have IoU 0 / 0: nothing is
    suppressed, whatever the threshold -- not even above 0."""
    two = [NC.unit_cube(0.0), NC.unit_cube(0.1)]
    assert hand(two, [np.nan, 0.1], [[0, 1]], [0.5], [0]) == [[0, 1]]            # the NaN box is ranked last and suppressed
    assert hand(two, [np.nan, -np.inf], [[0, 1]], [0.5], [0]) == [[1, 0]]        # a tie of keys: the lower index wins
    flat = (0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.3)
    for metric in NC.METRICS:
        keep = hand([flat, flat, NC.unit_cube(4.0), NC.unit_cube(4.1)], [0.9, 0.8, 0.7, 0.6], [[0, 1, 2, 3]], [0.0, 0.5, 1.0], [0, 1, 2], metric=metric)
        assert keep == [[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 1]], metric


def test_empty_calls_still_answer():
    rt = cpu_rt()
    k = np.stack([NC.corners_of(NC.unit_cube(0.0))] * 3)
    for offsets in ([0], [0, 0, 0]):                                # no group; empty groups only
        keep, n_kept = SW.run_nms_sweep(rt, k, np.ones(3, np.float32), offsets, [], [0.5], [0, -1], None, '3d')
        assert keep.shape == (2, 3) and not keep.any() and list(n_kept) == [0, 0]
    keep, n_kept = SW.run_nms_sweep(rt, k[:0], np.ones(0, np.float32), [0], [], [0.5], [0, -1], None, '3d')
    assert keep.shape == (2, 0) and list(n_kept) == [0, 0]


@pytest.mark.parametrize('metric', NC.METRICS)
def test_device_nms_sweep_on_the_specification_library(metric):
    """The plumbing of DeviceNmsSweep (strides, uploads, the view it returns) against per-configuration DeviceNms calls."""
    rt = cpu_rt()
    case = SW.repaired_case(metric, SW.GRID_K[4])
    keep, n_kept, ct, listed = SW.check_nms_sweep(rt, case, 7, 4, metric)
    n_members = len([b for g in case.groups for b in g])
    assert n_kept[0] == n_members and 0 < n_kept[3] < n_members      # (row 0: all listed, no threshold; row 3: all listed, above 0.5)
    SW.check_nms_sweep(rt, case, 3, 1, metric, with_listed=False)
    assert SW.moved_nms_sweep(rt, case, 7, 4, metric).tobytes() == keep.tobytes()
    with pytest.raises(ValueError):
        SW.run_nms_sweep(rt, *case.arrays(), [0.1] * 17, [0], None, metric)
    with pytest.raises(ValueError):
        SW.run_nms_sweep(rt, *case.arrays(), [0.5], [], None, metric)


# ---- hand cases: the evaluation -------------------------------------------------------------------------------------------------------
def test_eval_sweep_hand_case():
    """Two boxes in image 1.  Detections: a (0.9) on box 1; b (0.8) on box 1 too, a duplicate; c (0.7) on box 2; d (0.6) in an image without
    ground truth.  All: tp fp tp fp -> recall .5 .5 1 1, precision 1 1/2 2/3 1/2 -> 1/2 + 1/2 * 2/3 = 5/6.  Without a, b takes box 1:
    tp tp fp -> 1.  c alone: 1/2.  d alone, and nothing: 0."""
    shift = lambda x: SC.box(x, 5.0, 0.0, 1.0, 1.0, 1.0)
    det = SC.stack([shift(0.0), shift(0.1), shift(3.0), shift(0.0)], [1, 1, 1, 5], [0.9, 0.8, 0.7, 0.6])
    gt = SC.stack([shift(0.0), shift(3.0)], [1, 1])
    gt['classname'] = ['table', 'table']
    masks = np.asarray([[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]], np.uint8)
    r = ES.sweep_class('table', det, gt, masks, None, 0.25, cpu_rt())
    assert np.allclose(r['ap'], [5.0 / 6.0, 1.0, 0.5, 0.0, 0.0], atol=1e-15, rtol=0)
    assert list(r['n_det']) == [4, 3, 1, 1, 0] and list(r['n_tp']) == [2, 2, 1, 0, 0] and list(r['n_fp']) == [2, 1, 0, 1, 0]
    # the same rows read through det_index out of a wider matrix
    wide = np.zeros((5, 9), np.uint8)
    wide[:, [7, 2, 5, 0]] = masks
    wide[:, [1, 3, 4, 6, 8]] = 1
    q = ES.sweep_class('table', det, gt, wide, np.asarray([7, 2, 5, 0], np.int32), 0.25, cpu_rt())
    assert all(np.array_equal(r[k], q[k]) for k in r)
    with pytest.raises(ValueError):
        ES.sweep_class('table', det, gt, wide, np.asarray([7, 2, 5], np.int32), 0.25, cpu_rt())


@pytest.mark.parametrize('P,G,M,wide', [(0, 0, 1, False), (0, 3, 2, False), (1, 1, 1, False), (5, 0, 3, True), (40, 6, 5, False), (40, 6, 4, True)])
def test_eval_sweep_plumbing_on_the_specification_library(P, G, M, wide):
    print(SW.check_eval_sweep(cpu_rt(), P, G, M, wide=wide, exact=True))


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
def test_grid_order_values_and_errors():
    g = SWP.Grid(['0.5', 'off', '0.25', '0.5'], None, ['0.3'], ['off', '0.2', 'OFF'])
    assert g.values == {'nms_iou': [None, 0.5, 0.25], 'min_reproj_iou': [None], 'min_mask_in_box': [0.3], 'min_seg_box_iou': [None, 0.2]}
    assert g.rows == [(None, None, 0.3, None), (None, None, 0.3, 0.2), (0.5, None, 0.3, None), (0.5, None, 0.3, 0.2), (0.25, None, 0.3, None),
                      (0.25, None, 0.3, 0.2)]                                      # the product in flag order, the last flag fastest, off first
    assert g.thresholds == [0.5, 0.25] and g.consistency and (g.metric, g.score) == ('3d', 'prob') and len(g) == 6
    assert SWP.flags_text(g.rows[3]) == '--nms_iou 0.5 --min_mask_in_box 0.3 --min_seg_box_iou 0.2' and SWP.flags_text((None,) * 4) == '(no flags)'
    assert not SWP.Grid(['0.25']).consistency and SWP.Grid(['0.25'], nms_metric='bev', nms_score='score').metric == 'bev'
    assert SWP.Grid(None, ['off']).consistency                                      # given, if only as off: the measures are taken
    for bad in (dict(), dict(nms_iou=['0']), dict(nms_iou=['1.5']), dict(nms_iou=['x']), dict(min_reproj_iou=['-0.1']), dict(min_seg_box_iou=['nan']),
                dict(min_reproj_iou=['0.5'], nms_metric='bev'), dict(nms_iou=['off'], nms_score='score'), dict(nms_iou=['0.5'], nms_metric='2d'),
                dict(nms_iou=['%g' % (0.01 * k) for k in range(1, 18)]),           # 17 distinct NMS thresholds
                dict(nms_iou=['%g' % (0.05 * k) for k in range(1, 17)], min_reproj_iou=['%g' % (0.01 * k) for k in range(65)],
                     min_mask_in_box=['%g' % (0.01 * k) for k in range(64)])):     # 16 * 65 * 64 = 66560 configurations
        with pytest.raises(ValueError):
            SWP.Grid(**bad)
    assert len(SWP.Grid(['%g' % (0.05 * k) for k in range(1, 17)], ['%g' % (0.01 * k) for k in range(64)], ['%g' % (0.01 * k) for k in range(64)])) == 65536


def test_ranking_ties_in_grid_order_and_the_table():
    g = SWP.Grid(['off', '0.25', '0.5', '0.75'])
    classes = ES.CLASS_NAMES['B']
    ap = np.asarray([0.2, 0.5, 0.5, 0.1])
    per = {c: {'ap': ap.copy(), 'n_det': np.asarray([9, 7, 8, 9], np.int32), 'n_tp': np.asarray([2, 3, 3, 1], np.int32),
               'n_fp': np.asarray([7, 4, 5, 8], np.int32)} for c in classes}
    r = SWP.Result(g, classes, per, ap.copy(), np.asarray([45, 35, 40, 45]), 45, 0, 'B', 0.25)
    assert r.ranking() == [1, 2, 0, 3] and r.ranking(2) == [1, 2] and r.best()['flags'] == '--nms_iou 0.25'
    lines = r.lines(2)
    assert lines[0] == 'sweep: 4 configurations over 45 detections of 5 classes'
    assert lines[1] == 'baseline: mAP 20 | table 20.00 sofa 20.00 dresser 20.00 night_stand 20.00 bookshelf 20.00 | kept 45'
    assert lines[2].startswith('  1. --nms_iou 0.25: mAP 50 | table 50.00 ') and lines[2].endswith('| kept 35')
    assert lines[3].startswith('  2. --nms_iou 0.5: mAP 50 | ') and lines[4] == 'best: --nms_iou 0.25' and len(lines) == 5
    assert r.table()[3]['options'] == {'nms_iou': 0.75, 'min_reproj_iou': None, 'min_mask_in_box': None, 'min_seg_box_iou': None}
    assert r.table()[3]['n_fp']['sofa'] == 8 and r.baseline['index'] == 0


# ---- flags ----------------------------------------------------------------------------------------------------------------------------
def test_flag_errors(tmp_path):
    needed = ['--dataset_dir', str(tmp_path), '--idx_path', 'none', '--rgb_detection_path', 'none']
    sweep = ['--sweep', '--sweep_nms_iou', '0.25']
    for extra in (['--sweep'],                                                  # at least one --sweep_* list
                  ['--sweep_nms_iou', '0.25'], ['--sweep_json', 'x.json'], ['--sweep_top', '3'],      # ... which need --sweep
                  sweep + ['--nms_iou', '0.3'], sweep + ['--nms_fuse'], sweep + ['--nms_fuse_iou', '0.5'], sweep + ['--min_reproj_iou', '0.5'],
                  sweep + ['--min_mask_in_box', '0.5'], sweep + ['--min_seg_box_iou', '0.5'], sweep + ['--official_eval', '--diagnose'],
                  sweep + ['--vis_dir', str(tmp_path)], sweep + ['--consistency_json', 'x.json'], sweep + ['--sweep_top', '-1'],
                  ['--sweep', '--sweep_nms_iou', '0'], ['--sweep', '--sweep_nms_iou', 'of'], ['--sweep', '--sweep_min_reproj_iou', '1.5'],
                  ['--sweep', '--sweep_min_reproj_iou', '0.5', '--nms_metric', 'bev'],
                  ['--sweep', '--sweep_nms_iou'] + ['%g' % (0.01 * k) for k in range(1, 18)],
                  ['--sweep', '--sweep_nms_iou'] + ['%g' % (0.05 * k) for k in range(1, 17)] + ['--sweep_min_reproj_iou'] + ['%g' % (0.01 * k) for k in range(65)]
                  + ['--sweep_min_mask_in_box'] + ['%g' % (0.01 * k) for k in range(64)]):
        with pytest.raises(SystemExit):
            DT.main(needed + extra, log=lambda *a: None)
    grid = SWP.Grid(['0.25'], ['0.5'])
    from transferable3d_amd import test_semisup as TS
    import detect_check as DC
    rt = cpu_rt()
    flags = lambda: TS.build_flags(DC.MODEL_FLAGS)
    for kw in (dict(nms_iou=0.3), dict(min_reproj_iou=0.5), dict()):            # not the plain run; the measures are missing
        with pytest.raises(ValueError):
            DT.Detector(flags(), rt=rt, **kw).sweep_parts([], grid, str(tmp_path), [])
    with pytest.raises(ValueError, match='no detections'):
        DT.Detector(flags(), rt=rt, consistency=True).sweep_parts([], grid, str(tmp_path), [])


# ---- the flow -------------------------------------------------------------------------------------------------------------------------
def test_detect_sweep_equals_one_detect_run_per_row(tmp_path):
    print('\n'.join(SW.check_flow(cpu_rt(), tmp_path, exact=True)))
