"""CPU: box voting behind the per-scene NMS (t3d_detect_fuse, nms.DeviceFuse, detect --nms_fuse) on the NumPy specification
(tests/fake_fuse.py): hand cases whose answers need no code, degenerate inputs, the argument struct, the argument checks of the built
library, the flags, the conditions the generated cases of the GPU tests have to meet (same seeds), and the whole flow on the duplicated
golden scenes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fake_fuse as FF
import fake_nms as FN
import fuse_check as FC
import nms_check as NC
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from transferable3d_amd import abi, detect as DT, nms as NMS, semisup_infer as SI
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SpecLib(FF.DetectFuseSpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib):
    pass


def cpu_rt():
    return Runtime(device='cpu', lib=SpecLib())


def fuse(boxes, weights, groups, threshold, vote=None, metric='3d', scores=None, labels=None):
    """NMS and fusion of the specification on boxes (cx, cy, cz, l, w, h, ry) -> (keep, suppressed_by, label_out, corners_out, n_votes,
    label, corners)"""
    label = np.stack([FC.label_of(b) for b in boxes]) if labels is None else np.asarray(labels, np.float32)
    corners = np.stack([NC.corners_of(b) for b in boxes])
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    members = np.asarray([b for g in groups for b in g], np.int32)
    scores = weights if scores is None else scores
    keep, sup, rank = FN.greedy_nms(corners, np.asarray(scores, np.float32), offsets, members, threshold, NC.METRIC_ID[metric])
    lo, ko, nv, _ = FF.fuse_clusters(label, corners, np.asarray(weights, np.float32), offsets, members, keep, sup, rank,
                                     threshold if vote is None else vote, NC.METRIC_ID[metric])
    return keep, sup, lo, ko, nv, label, corners


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
def test_two_unit_cubes():
    """Anchor at the origin, weight 0.9; voter 0.2 along x, weight 0.6, IoU 0.8 / 1.2 = 2/3: the fused centre x is 0.6 * 2/3 * 0.2 / (0.9 +
    0.4) = 0.4 * 0.2 / 1.3, the dimensions stay 1."""
    keep, sup, lo, ko, nv, label, _ = fuse([NC.unit_cube(0.0), NC.unit_cube(0.2)], [0.9, 0.6], [[0, 1]], 0.25)
    assert list(keep) == [1, 0] and list(sup) == [-1, 0] and list(nv) == [1, -1]
    assert abs(lo[0][3] - 0.4 * 0.2 / 1.3) < 1e-6
    assert list(lo[0][:3]) == [1, 1, 1] and lo[0][4] == label[0][4] and lo[0][5] == label[0][5] and lo[0][6] == 0
    assert np.abs(ko[0] - NC.corners_of((0.4 * 0.2 / 1.3, 0.0, 3.0, 1, 1, 1, 0))).max() < 1e-6
    assert lo[1].tobytes() == label[1].tobytes()


def test_a_quarter_turn_with_l_and_w_exchanged_is_the_same_box():
    """(l, w, ry) = (2, 1, 0) and (1, 2, pi/2): a naive mean would give (1.5, 1.5)."""
    a, b = (0, 0, 3, 2, 1, 1, 0), (0, 0, 3, 1, 2, 1, np.pi / 2)
    assert abs(FN.iou_corners(NC.corners_of(a), NC.corners_of(b))[0] - 1) < 1e-6
    keep, sup, lo, ko, nv, label, corners = fuse([a, b], [0.9, 0.6], [[0, 1]], 0.25)
    assert list(nv) == [1, -1]
    assert list(lo[0][:6]) == list(label[0][:6]) and abs(lo[0][6]) < 1e-7        # (fp32 pi/2 is not pi/2: the heading moves by 2e-8)
    assert np.abs(ko[0] - corners[0]).max() < 1e-6
    assert FF.align(0.0, np.pi / 2)[0] in (1, 3) and FF.align(0.0, 0.1) == (0, 0.1)


def test_a_half_turn_is_the_same_heading():
    """Anchor ry = 0, voter ry = pi - 0.1: delta = -0.1, not pi - 0.1."""
    k, delta = FF.align(0.0, np.pi - 0.1)
    assert k == 2 and abs(delta + 0.1) < 1e-12
    a, b = (0, 0, 3, 2, 1, 1, 0), (0, 0, 3, 2, 1, 1, np.pi - 0.1)
    keep, sup, lo, _, nv, _, _ = fuse([a, b], [1.0, 1.0], [[0, 1]], 0.25)
    iou = FN.iou_corners(NC.corners_of(a), NC.corners_of(b))[0]
    assert list(nv) == [1, -1] and abs(lo[0][6] - (-0.1 * iou / (1 + iou))) < 1e-6 and list(lo[0][:3]) == [1, 1, 2]
    assert FF.wrap(np.pi) == np.pi and FF.wrap(-np.pi) == np.pi and abs(FF.wrap(3 * np.pi / 2) + np.pi / 2) < 1e-12


def test_a_vote_threshold_above_the_overlap_leaves_the_box_alone():
    keep, sup, lo, ko, nv, label, corners = fuse([NC.unit_cube(0.0), NC.unit_cube(0.2)], [0.9, 0.6], [[0, 1]], 0.25, vote=0.7)
    assert list(keep) == [1, 0] and list(nv) == [0, -1]
    assert lo.tobytes() == label.tobytes() and ko.tobytes() == corners.tobytes()


def test_chain_the_suppressed_box_votes_for_its_suppressor_only():
    """A > B > C, A covers B (IoU 0.6), B covers C, A and C overlap by 1/3: C is kept, and B votes for A only."""
    c = NC.cases('3d', 0.5)['chain']
    (keep, sup, rank), (lo, ko, nv), clusters = FC.expected(c, 0.5)
    label = FC.arrays(c)[0]
    assert list(keep) == [1, 0, 1] and list(nv) == [1, -1, 0] and sorted(clusters) == [0]
    assert abs(lo[0][3] - 0.8 * 0.6 * 0.25 / (0.9 + 0.8 * 0.6)) < 1e-6
    assert lo[2].tobytes() == label[2].tobytes() and lo[1].tobytes() == label[1].tobytes()


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------------
def test_weights_that_count_as_zero():
    boxes = [NC.unit_cube(0.0), NC.unit_cube(0.2), NC.unit_cube(0.1)]
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        # a bad voter weight: the voter is counted and changes nothing but through the other voter
        keep, sup, lo, _, nv, label, _ = fuse(boxes, [0.9, bad, 0.5], [[0, 1, 2]], 0.25, scores=[0.9, 0.6, 0.5])
        i2 = FN.iou_corners(NC.corners_of(boxes[0]), NC.corners_of(boxes[2]))[0]
        assert list(nv) == [2, -1, -1] and abs(lo[0][3] - 0.5 * i2 * 0.1 / (0.9 + 0.5 * i2)) < 1e-6
        # a bad anchor weight: the mean of the voters
        keep, sup, lo, _, nv, label, _ = fuse(boxes[:2], [bad, 0.6], [[0, 1]], 0.25, scores=[0.9, 0.6])
        assert list(nv) == [1, -1] and abs(lo[0][3] - 0.2) < 1e-6
        # nothing left: W = 0, byte copies, the voter still counted
        keep, sup, lo, ko, nv, label, corners = fuse(boxes[:2], [bad, bad], [[0, 1]], 0.25, scores=[0.9, 0.6])
        assert list(nv) == [1, -1] and lo.tobytes() == label.tobytes() and ko.tobytes() == corners.tobytes()


def test_non_finite_labels():
    boxes = [NC.unit_cube(0.0), NC.unit_cube(0.2), NC.unit_cube(0.1)]
    label = np.stack([FC.label_of(b) for b in boxes])
    for bad in (np.nan, np.inf):
        voter = label.copy()
        voter[1, 2] = bad                       # a voter's label: it does not vote
        keep, sup, lo, _, nv, _, _ = fuse(boxes, [0.9, 0.6, 0.5], [[0, 1, 2]], 0.25, labels=voter)
        assert list(nv) == [1, -1, -1] and np.isfinite(lo[0]).all() and lo[1].tobytes() == voter[1].tobytes()
        anchor = label.copy()
        anchor[0, 6] = bad                      # the anchor's own label: byte copies, nobody is asked
        keep, sup, lo, ko, nv, _, corners = fuse(boxes, [0.9, 0.6, 0.5], [[0, 1, 2]], 0.25, labels=anchor)
        assert list(nv) == [0, -1, -1] and lo.tobytes() == anchor.tobytes() and ko.tobytes() == corners.tobytes()


def test_zero_volume_ties_empty_groups_and_unlisted_boxes():
    for metric in NC.METRICS:
        c = NC.cases(metric, 0.25)['zero_volume']           # two boxes without extent (IoU 0 / 0), then two cubes
        _, (lo, ko, nv), clusters = FC.expected(c, 0.25)
        assert list(nv) == [0, 0, 1, -1] and sorted(clusters) == [2]
    c = NC.cases('3d', 0.5)['ties_nan']                     # score ties; NaN and -inf scores are the weights, which count as 0
    (keep, sup, rank), (lo, ko, nv), clusters = FC.expected(c, 0.5)
    label, corners = FC.arrays(c)[:2]
    assert list(nv) == [1, -1, -1, 1, 2, -1, -1] and sorted(clusters) == [0, 3]
    assert abs(lo[0][3] - 0.1 * (0.9 / 1.1) / (1 + 0.9 / 1.1)) < 1e-6           # a shift of 0.1, equal weights 0.5: the IoU alone tips the mean
    assert lo[3].tobytes() == label[3].tobytes()                                   # its only voter weighs 0: the mean of one box
    assert lo[4].tobytes() == label[4].tobytes() and ko[4].tobytes() == corners[4].tobytes()      # W = 0
    # empty groups, a group of one, unlisted boxes: all three outputs keep their fill values
    c = NC.cases('3d', 0.25)['mixed_40']
    _, (lo, ko, nv), _ = FC.expected(c, 0.25)
    u = np.asarray(c.unlisted)
    assert len(u) >= 4 and (lo[u] == FC.FILL[0]).all() and (ko[u] == FC.FILL[1]).all() and (nv[u] == FC.FILL[2]).all()
    one = NC.cases('3d', 0.25)['size_1']
    _, (lo, ko, nv), _ = FC.expected(one, 0.25)
    assert list(nv) == [0] and lo.tobytes() == FC.arrays(one)[0].tobytes()
    rt = cpu_rt()
    k = np.stack([NC.corners_of(NC.unit_cube(0.0))] * 3)
    l = np.stack([FC.label_of(NC.unit_cube(0.0))] * 3)
    for offsets in ([0], [0, 0, 0]):                        # no group; empty groups only
        _, got = FC.run(rt, l, k, np.ones(3, np.float32), offsets, [], 0.25, '3d', 0.25)
        assert all((g == f).all() for g, f in zip(got, FC.FILL))
    _, got = FC.run(rt, l[:0], k[:0], np.ones(0, np.float32), [0], [], 0.25, '3d', 0.25)
    assert all(len(g) == 0 for g in got)


# ---- the generated cases: their conditions, and DeviceFuse through the specification library -------------------------------------------
@pytest.mark.parametrize('metric,threshold,vote', FC.PASSES)
def test_generated_cases_keep_their_margins(metric, threshold, vote):
    """What the GPU tests rely on, on the seeds they use: both caps hold (asserted while the cases are built), no same-group IoU near T or
    V, no voter near a tie of the quarter turns, and every pass fuses something."""
    cs = dict(FC.cases(metric, threshold, vote))
    if (metric, threshold, vote) == ('3d', 0.25, 0.25):
        cs['group_1024'] = FC.big_case(metric, threshold)
    fused = 0
    for name, c in cs.items():
        assert c.redrawn <= NC.MAX_REDRAWN * c.n and (c.metric, c.threshold) == (metric, threshold)
        corners, score, offsets, members = c.arrays()
        pairs = {}
        for g in c.groups:
            FN.group_pairs(corners.astype(np.float64), score, np.asarray(g, np.int64), pairs, NC.memo_iou)
        ious = [v[NC.METRIC_ID[metric]] for v in pairs.values() if v[0] == v[0]]
        assert c.hand_built or all(abs(v - threshold) >= NC.MARGIN and abs(v - vote) >= NC.MARGIN for v in ious), name
        assert all(abs(v - vote) >= NC.MARGIN for v in ious), name
        assert c.hand_built or not FC.near_quarter(c, vote), name
        _, (lo, ko, nv), clusters = FC.expected_of(name, metric, threshold, vote)
        fused += len(clusters)
        if not c.hand_built and c.n > 2:
            assert clusters and (nv == 0).any(), name
    sizes = sorted(len(g) for c in cs.values() for g in c.groups)
    assert {0, 1, 2, 63, 64, 65, 130, 260} <= set(sizes) and fused > 50
    if vote > threshold:                            # the higher vote threshold turns some voters away
        low = sum(int(v[v > 0].sum()) for v in (FC.expected(c, threshold)[1][2] for c in cs.values()))
        high = sum(int(v[v > 0].sum()) for v in (FC.expected(c, vote)[1][2] for c in cs.values()))
        assert 0 < high < low


MOVED = ('mixed_40', 'size_65', 'chain', 'ties_nan', 'size_2', 'zero_volume')


@pytest.mark.parametrize('metric,threshold,vote', [('3d', 0.25, 0.25), ('bev', 0.5, 0.5), ('3d', 0.25, 0.6)])
def test_device_fuse_on_the_specification_library(metric, threshold, vote):
    rt = cpu_rt()
    for name in FC.cases(metric, threshold, vote):
        FC.check_case(rt, name, metric, threshold, vote)
    names = [k for k in MOVED if k in FC.cases(metric, threshold, vote)]
    for name, got in zip(names, FC.moved(rt, names, metric, threshold, vote)):
        want = FC.expected_of(name, metric, threshold, vote)[1]
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), name + ' moved'


# ---- the argument struct ---------------------------------------------------------------------------------------------------------------
def test_struct_follows_the_header_and_the_compiler(tmp_path):
    assert 't3d_detect_fuse' in abi.ENTRY_POINTS
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\}\s*t3d_detect_fuse_args;', h).group(1), flags=re.S)
    names = [re.findall(r'(\w+)\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]
    assert names == [f[0] for f in abi.DetectFuseArgs._fields_]
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "t3d.h"\nint main(void) { printf("%zu %d %llu %zu %zu %d\\n", '
                   'sizeof(t3d_detect_fuse_args), T3D_V2_SIZE_detect_fuse_args, (unsigned long long)T3D_DETECT_FUSE_WORKSPACE_BYTES(1001), '
                   'offsetof(t3d_detect_fuse_args, vote_threshold), offsetof(t3d_detect_fuse_args, n_votes), T3D_ABI_VERSION); return 0; }\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'size')])
    size, v2, ws, off_t, off_v, version = (int(v) for v in subprocess.check_output([str(tmp_path / 'size')], text=True).split())
    assert size == v2 == C.sizeof(abi.DetectFuseArgs) and abi.DetectFuseArgs().struct_size == size and version == 3
    assert ws == abi.detect_fuse_workspace_bytes(1001) == 4008 + 1001 * 16
    assert off_t == abi.DetectFuseArgs.vote_threshold.offset and off_v == abi.DetectFuseArgs.n_votes.offset


def full_args(buf, **kw):
    f, i = C.cast(buf, abi.F), C.cast(buf, abi.I)
    a = abi.DetectFuseArgs(n=10, n_groups=1, metric=0, group_offsets=i, members=i, keep=C.cast(buf, abi.U8), suppressed_by=i, rank=i, label=f,
                           corners=f, weight=f, vote_threshold=0.25, max_group=10, workspace=C.addressof(buf),
                           workspace_bytes=abi.detect_fuse_workspace_bytes(10), label_out=f, corners_out=f, n_votes=i)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('which', ['built', 'specification'])
def test_the_library_checks_before_it_launches(which):
    """No GPU needed: the struct size, the group size cap, the metric, the vote threshold, the pointers and the workspace are checked
    before anything is launched -- by the built library and, with the same answers, by the specification library."""
    lib, null = (abi.load() if which == 'built' else SpecLib()), C.c_void_p(0)
    call = lambda a: lib.t3d_detect_fuse(C.byref(a), null)
    a = abi.DetectFuseArgs()
    a.struct_size -= 8
    assert call(a) == abi.ERR_ABI
    assert call(abi.DetectFuseArgs()) == 0                                  # n == 0: nothing to do
    assert call(abi.DetectFuseArgs(n=5, n_groups=0, max_group=3)) == 0 and call(abi.DetectFuseArgs(n=5, n_groups=2, max_group=0)) == 0
    a = abi.DetectFuseArgs(n=2000, n_groups=1, metric=0, max_group=1025, vote_threshold=0.5)
    assert call(a) == -2                                                    # T3D_ERR_SHAPE
    a.max_group = 1024
    assert call(a) == -1                                                    # null pointers
    buf = (C.c_uint64 * 64)()
    for bad in (dict(metric=2), dict(metric=-1), dict(vote_threshold=-0.01), dict(vote_threshold=1.01), dict(vote_threshold=float('nan')),
                dict(n=-1), dict(n_groups=-1), dict(max_group=-1), dict(workspace_bytes=abi.detect_fuse_workspace_bytes(10) - 8),
                dict(workspace=C.addressof(buf) + 4)):
        assert call(full_args(buf, **bad)) == -1, bad
    for k in ('group_offsets', 'members', 'keep', 'suppressed_by', 'rank', 'label', 'corners', 'weight', 'workspace', 'label_out',
              'corners_out', 'n_votes'):
        assert call(full_args(buf, **{k: None})) == -1, k


def test_a_group_of_1025_is_refused_through_device_fuse():
    big = np.zeros((1025, 8, 3), np.float32)
    with pytest.raises(abi.T3DError, match='T3D_ERR_SHAPE'):
        FC.run(cpu_rt(), np.zeros((1025, 7), np.float32), big, np.zeros(1025, np.float32), [0, 1025], np.arange(1025), 0.25, '3d', 0.25)


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def test_flag_errors(tmp_path):
    assert NMS.check_fuse_options(None) == (False, None) and NMS.check_fuse_options(0.3) == (False, None)
    assert NMS.check_fuse_options(0.3, True) == (True, 0.3) and NMS.check_fuse_options(0.3, False, 0.5) == (True, 0.5)
    assert NMS.check_fuse_options(0.3, True, 0.3) == (True, 0.3) and NMS.check_fuse_options(0.3, True, 1.0) == (True, 1.0)
    for bad in ((None, True, None), (None, False, 0.5), (0.3, True, 0.29), (0.3, False, 1.01), (0.3, True, float('nan'))):
        with pytest.raises(ValueError):
            NMS.check_fuse_options(*bad)
    assert NMS.check_options(0.3) == (0.3, '3d', 'prob')                    # (as it was)
    for kw in (dict(nms_fuse=True), dict(nms_fuse_iou=0.5), dict(nms_iou=0.3, nms_fuse_iou=0.2), dict(nms_iou=0.3, nms_fuse=True, nms_fuse_iou=1.5)):
        with pytest.raises(ValueError):
            DT.Detector(object(), **kw)
    needed = ['--dataset_dir', str(tmp_path), '--idx_path', 'none', '--rgb_detection_path', 'none']
    for extra in (['--nms_fuse'], ['--nms_fuse_iou', '0.5'], ['--nms_iou', '0.3', '--nms_fuse_iou', '0.25'],
                  ['--nms_iou', '0.3', '--nms_fuse', '--nms_fuse_iou', '1.01']):
        with pytest.raises(SystemExit):
            DT.main(needed + extra, log=lambda *a: None)
    dev = ['--device_decode', '--from_rgb_detection']
    f = SI.build_flags(dev + ['--nms_iou', '0.3', '--nms_fuse'])
    assert (f.nms_fuse, f.nms_fuse_iou) == (True, 0.3)
    f = SI.build_flags(dev + ['--nms_iou', '0.3', '--nms_fuse_iou', '0.5'])
    assert (f.nms_fuse, f.nms_fuse_iou) == (True, 0.5)
    assert SI.build_flags(dev + ['--nms_iou', '0.3']).nms_fuse is False and SI.build_flags([]).nms_fuse is False
    for argv in (dev + ['--nms_fuse'], dev + ['--nms_fuse_iou', '0.5'], dev + ['--nms_iou', '0.3', '--nms_fuse_iou', '0.2'],
                 ['--nms_iou', '0.3', '--nms_fuse']):
        with pytest.raises(ValueError):
            SI.build_flags(argv)
    r = SI.NmsRequest(0.3, None, None, [1], [2], [0.5], fuse=True)
    assert (r.fuse, r.vote_threshold) == (True, 0.3) and SI.NmsRequest(0.3, None, None, [1], [2], [0.5]).fuse is False
    with pytest.raises(ValueError):
        SI.NmsRequest(0.3, None, None, [1], [2], [0.5], vote_threshold=0.1)


# ---- the flow --------------------------------------------------------------------------------------------------------------------------
def test_detect_with_fusion_equals_the_spec_on_the_plain_run_and_the_two_step_route(tmp_path):
    print('\n'.join(FC.check_flow(cpu_rt(), tmp_path, exact=True)))


def test_vis_dir_draws_the_fused_boxes_and_says_how_many_voted(tmp_path):
    """--vis_dir with --nms_fuse: the legend entries of kept boxes gain 'votes', the result files are those of the run without pictures,
    and t3d_render is handed the fused corners for the kept boxes and the decode's own for the grey ones of --vis_suppressed."""
    import json
    import detect_check as DC
    import fake_render as FR
    from transferable3d_amd import test_semisup as TS

    seen = []

    class VisLib(FR.RenderSpec, SpecLib):
        def t3d_render(self, a, stream):
            p = a._obj
            seen.append(np.ctypeslib.as_array(p.corners, shape=(p.n_corner_boxes, 8, 3)).copy())
            return super().t3d_render(a, stream)

    rt, quiet = Runtime(device='cpu', lib=VisLib()), (lambda *a: None)
    ids, folder, idx, dets = NC.write_duplicated(tmp_path)
    base = ['--dataset_dir', str(tmp_path), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS + ['--nms_iou', str(NC.FLOW_T), '--nms_fuse']
    res = lambda name: os.path.join(str(tmp_path), name)
    DT.main(base + ['--result_dir', res('fuse')], rt=rt, log=quiet)
    assert not seen
    DT.main(base + ['--result_dir', res('fuse_vis'), '--vis_dir', res('pics'), '--vis_suppressed'], rt=rt, log=quiet)
    assert DC.read_results(res('fuse_vis')) == DC.read_results(res('fuse'))
    scenes = DC.load_scenes(tmp_path, ids)
    det = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, nms_iou=NC.FLOW_T, nms_fuse=True)
    meta, d = det.decode_all([det.extract(scenes, dets, ids)])
    assert seen and all(np.array_equal(k[:len(d)], d.corners.astype(np.float32)) for k in seen)      # the table t3d_render read (then a batch's padding)
    assert (d.n_votes > 0).any() and not np.array_equal(d.corners, d.raw_corners)
    assert np.array_equal(d.corners[~d.keep], d.raw_corners[~d.keep])                            # a grey box is the decode's own
    votes = []
    for s in ids:
        legend = json.load(open(os.path.join(res('pics'), '%06d.json' % s)))
        kinds = [b['kind'] for b in legend['boxes']]
        assert 'kept' in kinds and 'suppressed' in kinds
        assert all(b['votes'] == -1 for b in legend['boxes'] if b['kind'] == 'suppressed')
        votes += [b['votes'] for b in legend['boxes'] if b['kind'] == 'kept']
    assert votes == [int(v) for v in d.n_votes[d.keep]] and max(votes) > 0
