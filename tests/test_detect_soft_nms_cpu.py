"""CPU: Soft-NMS (t3d_detect_soft_nms, transferable3d_amd/nms.py DeviceSoftNms, detect --soft_nms) on the NumPy specification
(tests/fake_soft_nms.py): the rule on hand-computed numbers and its edge cases, its equality with the hard suppression where every decay
prunes, the usability of the shared cases (tests/soft_nms_check.py) on the seeds the GPU tests use, the argument struct, the flags, the
whole flow on the golden scenes, and one constructed scene that shows what the decay is for."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fake_consistency as FK
import fake_ensemble as FE
import fake_nms as FN
import fake_soft_nms as FS
import nms_check as NC
import soft_nms_check as SC
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from fake_render import RenderSpec
from fake_sunrgbd_eval import FakeSunrgbdEvalLib
from transferable3d_amd import abi, detect as DT, evaluate_sunrgbd as ES, nms as NMS, semisup_infer as SI
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SpecLib(FS.DetectSoftNmsSpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib, FakeSunrgbdEvalLib):
    pass


def cpu_rt():
    return Runtime(device='cpu', lib=SpecLib())


def spec_of(name, pass_id):
    return SC.cases(pass_id)[name].want


# ---- the rule, on numbers known by hand ------------------------------------------------------------------------------------------------
def test_chain_in_closed_form():
    """A 0.9, B 0.8, C 0.7; IoU(A,B) = IoU(B,C) = 3/5, IoU(A,C) = 1/3 under both metrics.  A is selected; B and C decay; C, the neighbour,
    now leads B, the duplicate, is selected and decays B again."""
    e = math.exp
    w = spec_of('chain', 0)                                   # gaussian, sigma 0.5
    assert np.allclose(w.score_out, [0.9, 0.8 * e(-0.72) * e(-0.72), 0.7 * e(-(1 / 9.0) / 0.5)], rtol=1e-6, atol=0)
    assert list(w.keep) == [1, 1, 1] and list(w.suppressed_by) == [-1, -1, -1] and list(w.n_decays) == [0, 2, 1]
    w = spec_of('chain', 1)                                   # gaussian, sigma 0.25, floor 0.05: B falls to 0.8 e^-2.88 = 0.045 at its second decay
    assert np.allclose(w.score_out, [0.9, 0.8 * e(-1.44) * e(-1.44), 0.7 * e(-(1 / 9.0) / 0.25)], rtol=1e-6, atol=0)
    assert list(w.keep) == [1, 0, 1] and list(w.suppressed_by) == [-1, 2, -1] and list(w.n_decays) == [0, 2, 1]
    w = spec_of('chain', 2)                                   # linear above 0.25: all three pairs decay
    assert np.allclose(w.score_out, [0.9, 0.8 * 0.4 * 0.4, 0.7 * (2 / 3.0)], rtol=1e-6, atol=0)
    assert list(w.keep) == [1, 1, 1] and list(w.n_decays) == [0, 2, 1]
    w = spec_of('chain', 3)                                   # linear above 0.5: A does not reach C
    assert np.allclose(w.score_out, [0.9, 0.8 * 0.4 * 0.4, 0.7], rtol=1e-6, atol=0)
    assert list(w.keep) == [1, 1, 1] and list(w.n_decays) == [0, 2, 0]
    assert w.bound[2] == 0 and w.bound[0] == 0 and w.bound[1] > 0


def test_edge_cases_of_the_rule():
    # scores that are not finite numbers above 0 take no part: they decay nothing, nothing decays them, they come back kept
    for p in range(len(SC.PASSES)):
        w = spec_of('ties_nan', p)
        assert list(w.keep) == [1] * 7 if SC.PASSES[p][4] < 0.05 else list(w.keep[2:]) == [1] * 5
        assert list(w.n_decays) == [0, 1, 0, 0, 0, 0, 0] and list(w.suppressed_by[2:]) == [-1] * 5      # equal scores: 0 is selected, 1 decays
        assert np.isnan(w.score_out[2]) and w.score_out[3] == np.float32(0.1) and w.score_out[4] == -np.inf and np.isnan(w.score_out[5])
        # a NaN IoU (two boxes without volume) decays nothing; the two cubes beside them still decay
        w = spec_of('zero_volume', p)
        assert list(w.n_decays) == [0, 0, 0, 1] and w.score_out[1] == np.float32(0.8) and w.bound[1] == 0
    # identical boxes, IoU 1: linear takes the lower one to 0, which any floor above 0 prunes; a floor of 0 keeps it (0 < 0 is false)
    k, s, off, mem = SC.cases(2)['identical'].arrays()
    w = FS.soft_nms(k, s, off, mem, 'linear', 0.25, min_score=0.0)
    assert abs(w.score_out[0]) < 1e-12 and w.keep[0] == 1 and w.n_decays[0] == 1
    w = spec_of('identical', 2)
    assert w.keep[0] == 0 and w.suppressed_by[0] == 1 and w.keep[2] == 1
    # zero, negative and infinite scores next to a live box; a box below the floor that nothing overlaps keeps its bits
    k = np.stack([NC.corners_of(NC.unit_cube(d)) for d in (0.0, 0.1, 0.2, 0.3, 5.0)])
    w = FS.soft_nms(k, np.asarray([0.9, 0.0, -0.5, np.inf, 1e-5], np.float32), [0, 5], [0, 1, 2, 3, 4], 'gaussian', min_score=0.05)
    assert list(w.keep) == [1] * 5 and list(w.n_decays) == [0] * 5 and list(w.score_out) == [np.float32(0.9), 0.0, -0.5, np.inf, np.float32(1e-5)]
    # a box listed in no group keeps the fill
    w = FS.soft_nms(k, np.ones(5, np.float32), [0, 2], [0, 1], 'gaussian', fill=SC.FILL)
    assert list(w.score_out[2:]) == [SC.FILL[0]] * 3 and list(w.keep[2:]) == [SC.FILL[1]] * 3 and list(w.n_decays[2:]) == [SC.FILL[3]] * 3
    assert w.n_decays[1] == 1 and w.score_out[0] == 1.0


@pytest.mark.parametrize('metric,threshold', NC.COMBOS)
def test_linear_with_a_floor_above_every_score_is_the_hard_suppression(metric, threshold):
    """Consequence (a), against the specification of t3d_detect_nms, on every case."""
    for name, c in list(NC.cases(metric, threshold).items()) + [('group_1024', NC.big_case(metric, threshold))] * (threshold == 0.25):
        k, s, off, mem = c.arrays()
        w = FS.soft_nms(k, s, off, mem, 'linear', threshold, min_score=2.0, metric=NC.METRIC_ID[metric], fill=SC.FILL, iou=NC.memo_iou)
        SC.hard_equal((w.score_out, w.keep, w.suppressed_by, w.n_decays), NC.expected(name, metric, threshold), s, mem, name)
        assert w.n_decays[mem].max(initial=0) <= 1


# ---- the shared cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pass_id', range(len(SC.PASSES)))
def test_the_shared_cases_are_usable(pass_id):
    """Building them asserts the conditions of soft_nms_check (no decision inside the bound, the redraw budget, something decayed, kept
    and -- at the 0.05 floor -- pruned); the originals of nms_check stay as they were."""
    before = {n: (c.arrays()[1].tobytes(), c.arrays()[0].tobytes()) for n, c in NC.cases(*SC.base_cases(pass_id)).items()}
    cs = SC.cases(pass_id)
    assert {n: (c.arrays()[1].tobytes(), c.arrays()[0].tobytes()) for n, c in NC.cases(*SC.base_cases(pass_id)).items()} == before
    sizes = sorted(len(g) for c in cs.values() for g in c.groups)
    assert {0, 1, 2, 63, 64, 65, 130, 260} <= set(sizes) and len(cs['mixed_40'].c.unlisted) >= 4 and set(SC.HAND) <= set(cs)
    for name, c in cs.items():
        assert c.redrawn <= NC.MAX_REDRAWN * c.n and not c.want.unsafe, name
        rel = c.want.bound / np.maximum(np.abs(c.want.score_out), 1e-300)
        print('%s: %d boxes, %d scores redrawn, %d boxes drawn again by the rejection step, floor %g, %d decayed, %d pruned, largest relative bound %.3g' % (
            name, c.n, c.redrawn, c.settled, c.floor, int((c.want.n_decays > 0).sum()), int((c.want.keep == 0).sum()),
            float(rel[(c.want.bound > 0) & (c.want.score_out != 0)].max(initial=0))))
        assert not c.want.slivers and not any(c.edge_pairs(g) for g in c.groups if SC.PASSES[pass_id][1] == 'gaussian' and not c.hand_built), name
        assert c.floor_raised == (c.floor != SC.PASSES[pass_id][4]) and (not c.floor_raised or len([b for g in c.groups for b in g]) == 2), name
    if pass_id in SC.BIG_PASSES:
        c = SC.big_case(pass_id)
        assert len(c.groups[0]) == abi.DETECT_NMS_MAX_GROUP and c.redrawn <= NC.MAX_REDRAWN * c.n


MOVED = ('mixed_40', 'size_65', 'chain', 'ties_nan', 'size_2', 'zero_volume')


@pytest.mark.parametrize('pass_id', range(len(SC.PASSES)))
def test_device_soft_nms_on_the_specification_library(pass_id):
    rt = cpu_rt()
    for name, c in SC.cases(pass_id).items():
        SC.check_case(SC.run_case(rt, c), c)
    for name, got in zip(MOVED, SC.moved(rt, MOVED, pass_id)):
        c = SC.cases(pass_id)[name]
        SC.check_case(got, c, name + ' moved', want=c.want_at_pass_floor)
    # linear with a floor of 2 through the library and DeviceNms through its own: consequence (a) end to end
    metric, method, threshold, _, _ = SC.PASSES[pass_id]
    if method == 'linear':
        for name, c in NC.cases(metric, threshold).items():
            k, s, off, mem = c.arrays()
            SC.hard_equal(SC.run(rt, k, s, off, mem, pass_id, floor=2.0), NC.run_case(rt, c), s, mem, name)


def test_empty_inputs_and_relaunch():
    rt = cpu_rt()
    none = np.zeros((0, 8, 3), np.float32), np.zeros(0, np.float32)
    assert all(len(a) == 0 for a in SC.run(rt, *none, [0], [], 0))
    k = np.stack([NC.corners_of(NC.unit_cube(0.0))] * 3)
    for offsets in ([0], [0, 0, 0]):                                    # no group at all; empty groups only
        got = SC.run(rt, k, np.ones(3, np.float32), offsets, [], 0)
        assert all((g == f).all() for g, f in zip(got, SC.FILL))
    dev = NMS.DeviceSoftNms(rt)
    c = SC.cases(0)['size_63']
    first = SC.run(rt, *c.arrays(), 0, dev=dev)
    dev.relaunch()                                                       # every listed box starts again from its input score
    again = tuple(t.cpu().numpy() for t in (dev.score_out[:c.n], dev.keep[:c.n], dev.suppressed_by[:c.n], dev.n_decays[:c.n]))
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    out = dev.run(rt.zeros(3, 24) + torch_of(k, rt), rt.zeros(3) + 1.0, [0, 2], [0, 1], 'gaussian')      # default fill: an unlisted box is kept, undecayed
    assert float(out[0][2]) == 1.0 and int(out[1][2]) == 1 and int(out[2][2]) == -1 and int(out[3][2]) == 0


def torch_of(a, rt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.reshape(len(a), -1))).to(rt.device)


# ---- the argument struct ---------------------------------------------------------------------------------------------------------------
def test_struct_follows_the_header_and_the_compiler(tmp_path):
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\}\s*t3d_detect_soft_nms_args;', h).group(1), flags=re.S)
    names = [re.findall(r'(\w+)\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]
    assert names == [f[0] for f in abi.DetectSoftNmsArgs._fields_]
    hard = [f[0] for f in abi.DetectNmsArgs._fields_]
    assert names[:hard.index('max_group') + 1] == hard[:hard.index('max_group') + 1]          # the leading fields of t3d_detect_nms_args
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "t3d.h"\nint main(void) { printf("%zu %d %llu %d %d %zu %zu\\n", '
                   'sizeof(t3d_detect_soft_nms_args), T3D_V2_SIZE_detect_soft_nms_args, (unsigned long long)T3D_DETECT_SOFT_NMS_WORKSPACE_BYTES(1001, 130), '
                   'T3D_SOFT_NMS_GAUSSIAN, T3D_SOFT_NMS_LINEAR, offsetof(t3d_detect_soft_nms_args, max_group), offsetof(t3d_detect_nms_args, max_group)); return 0; }\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'size')])
    size, v2, ws, g, l, o_soft, o_hard = (int(v) for v in subprocess.check_output([str(tmp_path / 'size')], text=True).split())
    assert size == v2 == C.sizeof(abi.DetectSoftNmsArgs) and abi.DetectSoftNmsArgs().struct_size == size and o_soft == o_hard
    assert ws == abi.detect_soft_nms_workspace_bytes(1001, 130) and (g, l) == (abi.SOFT_NMS_GAUSSIAN, abi.SOFT_NMS_LINEAR) == (FS.GAUSSIAN, FS.LINEAR)
    assert NMS.SOFT_METHODS == tuple(abi.SOFT_NMS_METHODS)


def test_both_libraries_check_before_they_launch():
    """No GPU needed: the struct size, the options, the group size cap and the pointers are checked before anything is launched."""
    null = C.c_void_p(0)
    buf = (C.c_uint64 * 64)()
    f, i = C.cast(buf, abi.F), C.cast(buf, abi.I)
    for lib in (abi.load(), SpecLib()):
        a = abi.DetectSoftNmsArgs()
        a.struct_size -= 8
        assert lib.t3d_detect_soft_nms(C.byref(a), null) == abi.ERR_ABI
        ok = dict(n=2000, n_groups=1, metric=0, max_group=1024, method=abi.SOFT_NMS_GAUSSIAN, sigma=0.5, min_score=0.001)
        assert lib.t3d_detect_soft_nms(C.byref(abi.DetectSoftNmsArgs(**dict(ok, max_group=1025))), null) == -2      # T3D_ERR_SHAPE
        assert lib.t3d_detect_soft_nms(C.byref(abi.DetectSoftNmsArgs(**ok)), null) == -1                             # null pointers
        full = dict(ok, corners=f, score=f, group_offsets=i, members=i, score_out=f, keep=C.cast(buf, abi.U8), suppressed_by=i)
        assert lib.t3d_detect_soft_nms(C.byref(abi.DetectSoftNmsArgs(**full)), null) == -1                           # n_decays still null
        full['n_decays'] = i
        for bad in (dict(metric=2), dict(method=2), dict(method=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float('inf')),
                    dict(sigma=float('nan')), dict(min_score=-0.001), dict(min_score=float('nan')), dict(n=-1), dict(max_group=-1)):
            assert lib.t3d_detect_soft_nms(C.byref(abi.DetectSoftNmsArgs(**dict(full, **bad))), null) == -1, bad
        # sigma is not read with linear; an empty call is valid
        assert lib.t3d_detect_soft_nms(C.byref(abi.DetectSoftNmsArgs(**dict(ok, method=abi.SOFT_NMS_LINEAR, sigma=0.0, n=0))), null) == 0
        assert lib.t3d_detect_soft_nms(C.byref(abi.DetectSoftNmsArgs(sigma=0.5)), null) == 0                         # n == 0: nothing to do
        assert lib.t3d_detect_soft_nms(C.byref(abi.DetectSoftNmsArgs()), null) == -1                                  # (gaussian with sigma 0)
    big = np.zeros((1025, 8, 3), np.float32)
    with pytest.raises(abi.T3DError, match='T3D_ERR_SHAPE'):
        SC.run(cpu_rt(), big, np.ones(1025, np.float32), [0, 1025], np.arange(1025), 0)


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def test_flag_errors(tmp_path):
    ok = NMS.check_soft_options
    assert ok(None) is None and ok('gaussian') == ('gaussian', None, 0.5, 0.001, '3d')
    assert ok('gaussian', 0.3, 0.0, nms_metric='bev') == ('gaussian', None, 0.3, 0.0, 'bev')
    assert ok('linear', None, 0.05, 0.25) == ('linear', 0.25, 0.5, 0.05, '3d')
    bad = (dict(soft_nms='cosine'), dict(soft_nms='gaussian', nms_iou=0.3), dict(soft_nms='linear'), dict(soft_nms='linear', nms_iou=1.5),
           dict(soft_nms='gaussian', nms_score='score'), dict(soft_nms='gaussian', nms_fuse=True), dict(soft_nms='linear', nms_iou=0.3, nms_fuse_iou=0.5),
           dict(soft_nms='gaussian', soft_nms_sigma=0.0), dict(soft_nms='gaussian', soft_nms_sigma=float('inf')), dict(soft_nms='gaussian', soft_nms_sigma=float('nan')),
           dict(soft_nms='linear', nms_iou=0.3, soft_nms_sigma=0.5), dict(soft_nms='gaussian', soft_nms_min_prob=1.0), dict(soft_nms='gaussian', soft_nms_min_prob=-0.1),
           dict(soft_nms='gaussian', soft_nms_min_prob=float('nan')), dict(soft_nms='gaussian', nms_metric='xy'), dict(soft_nms_sigma=0.5), dict(soft_nms_min_prob=0.1))
    for kw in bad:
        with pytest.raises(ValueError):
            ok(**kw)
        with pytest.raises(ValueError):                                    # before a model is built: FLAGS is never looked at
            DT.Detector(object(), **kw)
    needed = ['--dataset_dir', str(tmp_path), '--idx_path', 'none', '--rgb_detection_path', 'none']
    dev = ['--device_decode', '--from_rgb_detection']
    errors = (['--soft_nms', 'gaussian', '--nms_iou', '0.3'], ['--soft_nms', 'linear'], ['--soft_nms', 'gaussian', '--nms_score', 'score'],
              ['--soft_nms', 'gaussian', '--nms_fuse'], ['--soft_nms', 'linear', '--nms_iou', '0.3', '--nms_fuse_iou', '0.5'],
              ['--soft_nms_sigma', '0.5'], ['--soft_nms_min_prob', '0.01'], ['--soft_nms', 'gaussian', '--soft_nms_sigma', '0'],
              ['--soft_nms', 'gaussian', '--soft_nms_min_prob', '1'], ['--soft_nms', 'cosine'])
    for extra in errors + (['--soft_nms', 'gaussian', '--sweep'], ['--soft_nms', 'linear', '--nms_iou', '0.3', '--sweep']):
        with pytest.raises(SystemExit):
            DT.main(needed + extra, log=lambda *a: None)
    for extra in errors:
        with pytest.raises((ValueError, SystemExit)):
            SI.build_flags(dev + extra)
    for argv in (['--soft_nms', 'gaussian'], ['--from_rgb_detection', '--soft_nms', 'gaussian'], ['--device_decode', '--soft_nms', 'gaussian']):
        with pytest.raises(ValueError):
            SI.build_flags(argv)
    F = SI.build_flags(dev + ['--soft_nms', 'linear', '--nms_iou', '0.3', '--nms_metric', 'bev', '--soft_nms_min_prob', '0.05'])
    assert F.soft_nms == ('linear', np.float64(0.3), 0.5, 0.05, 'bev') and F.nms_iou is None and not F.nms_fuse
    assert SI.build_flags(dev).soft_nms is None and SI.build_flags([]).soft_nms is None
    req = SI.NmsRequest(None, 'bev', None, [1, 1], [2, 2], [0.5, 0.4], soft='gaussian', sigma=0.3)
    assert req.soft == ('gaussian', None, 0.3, 0.001, 'bev') and not req.fuse and req.score == 'prob'
    with pytest.raises(ValueError):
        SI.NmsRequest(None, None, None, [1], [2], None, soft='gaussian')        # the decay acts on `prob`
    with pytest.raises(ValueError):
        SI.inference(None, None, None, None, 4, decode='host', nms=req)
    with pytest.raises(ValueError, match='soft_nms'):
        DT.Detector.sweep_parts(type('D', (), dict(nms_iou=None, soft_nms=req.soft, suppression=NMS.suppression('gaussian', 0.3, nms_metric='bev'),
                                                   thresholds=(None,) * 3, tta=None))(), [], None, None, None)


# ---- the flow --------------------------------------------------------------------------------------------------------------------------
def test_detect_with_soft_nms_equals_the_spec_on_the_plain_run_and_the_two_step_route(tmp_path):
    print('\n'.join(SC.check_flow(cpu_rt(), tmp_path, exact=True)))


class StagesLib(FS.DetectSoftNmsSpec, FE.DetectEnsembleSpec, FK.ConsistencySpec, RenderSpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib,
                FakeSunrgbdEvalLib):
    pass


def test_soft_nms_beside_the_views_the_consistency_measures_and_the_pictures(tmp_path):
    print('\n'.join(SC.check_stages(Runtime(device='cpu', lib=StagesLib()), tmp_path)))


# ---- what it is for --------------------------------------------------------------------------------------------------------------------
def test_a_row_of_chairs_each_reported_twice():
    """Six unit cubes half an edge apart (neighbours overlap at IoU 1/3 > T = 0.25), each reported a second time a twentieth of an edge
    off and 0.05 lower in confidence, scored by the evaluation's specification at its 0.25 overlap.  Without suppression every duplicate
    is a false positive ahead of the next chair; the hard suppression at T removes the duplicates and every second chair with them;
    Soft-NMS sends the duplicates to the tail and keeps all six.  A property of this construction, not a SUN-RGBD result."""
    T, n = 0.25, 6
    shift = [0.5 * k + d for k in range(n) for d in (0.0, 0.05)]
    prob = np.asarray([0.9 - 0.1 * k - d for k in range(n) for d in (0.0, 0.05)], np.float32)
    corners = np.stack([NC.corners_of(NC.unit_cube(x)) for x in shift])
    offsets, members = NMS.groups_of([7] * len(shift), [3] * len(shift))
    cube = lambda xs, score: ES.boxes_from_label_format([7] * len(xs), *[np.full(len(xs), 1.0)] * 3, np.asarray(xs), np.zeros(len(xs)),
                                                        np.full(len(xs), 3.0), np.zeros(len(xs)), score)
    gt = cube([0.5 * k for k in range(n)], np.zeros(n))
    gt.pop('confidence')
    rt = cpu_rt()

    def ap(keep, score):
        rows = np.nonzero(keep)[0]
        return ES.compute_pr_curve_3d('chair', cube([shift[i] for i in rows], np.asarray(score, np.float64)[rows]), gt, threshold=0.25, rt=rt)['apScore']

    none = ap(np.ones(len(shift), bool), prob)
    hard = ap(FN.greedy_nms(corners, prob, offsets, members, T)[0], prob)
    soft = {}
    for method, kw in (('gaussian', dict(sigma=0.5)), ('linear', dict(threshold=T))):
        w = FS.soft_nms(corners, prob, offsets, members, method, min_score=0.001, **kw)
        soft[method] = ap(w.keep, w.score_out)
    print('AP without suppression %.4f, hard NMS at %.2f %.4f, Soft-NMS gaussian %.4f, linear %.4f' % (none, T, hard, soft['gaussian'], soft['linear']))
    assert abs(none - sum((k + 1) / (2 * k + 1.0) for k in range(n)) / n) < 1e-9 and abs(hard - 0.5) < 1e-9
    for v in soft.values():
        assert v >= hard and v >= none and (v > hard or v > none)
    assert abs(soft["gaussian"] - 1.0) < 1e-9
