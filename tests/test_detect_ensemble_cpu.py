"""CPU: test-time augmentation of `detect` (t3d_detect_ensemble, ensemble.DeviceEnsemble, detect --tta) on the NumPy specification
(tests/fake_ensemble.py): hand cases whose answers need no code, the mirror against an independent definition, degenerate inputs, the
argument struct, the argument checks of the built library, the flags, the conditions the generated cases of the GPU tests have to meet
(same seeds), and the whole flow on the golden scenes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import consistency_check as CC
import detect_check as DC
import ensemble_check as EC
import fake_consistency as FK
import fake_ensemble as FE
import fake_fuse as FF
import fake_nms as FN
import fuse_check as FC
import nms_check as NC
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from fake_render import RenderSpec
from fake_sunrgbd_eval import FakeSunrgbdEvalLib
from transferable3d_amd import abi, autolabel as AL, detect as DT, ensemble as EN, semisup_infer as SI, test_semisup as TS
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SpecLib(FE.DetectEnsembleSpec, FK.ConsistencySpec, RenderSpec, FF.DetectFuseSpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib,
              FakeSunrgbdEvalLib):
    pass


def cpu_rt():
    return Runtime(device='cpu', lib=SpecLib())


def ens(views, weights, vote=0.0, metric='3d', flip_mask=0, rot=None):
    """The specification on one detection whose views are boxes (cx, cy, cz, l, w, h, ry); a mirrored view is stored mirrored."""
    c = EC.hand_case('hand', [list(views)], [list(weights)], flip_mask, rot)
    return c, c.expected(metric, vote)


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
def test_two_unit_cubes():
    """View 0 at the origin, weight 0.9; view 1 0.2 along x, weight 0.6, IoU 0.8 / 1.2 = 2/3: two views tie, the anchor is view 0 and the
    fused centre x is 0.6 * 2/3 * 0.2 / (0.9 + 0.4); agreement and min_iou are that IoU."""
    c, w = ens([NC.unit_cube(0.0), NC.unit_cube(0.2)], [0.9, 0.6])
    assert w['anchor'][0] == 0 and w['n_votes'][0] == 1
    assert abs(w['agreement'][0] - 2 / 3) < 1e-6 and abs(w['min_iou'][0] - 2 / 3) < 1e-6
    lo = w['label_out'][0]
    assert abs(lo[3] - 0.4 * 0.2 / 1.3) < 1e-6 and list(lo[:3]) == [1, 1, 1] and lo[4] == c.labels[0, 0, 4] and lo[6] == 0
    assert np.abs(w['corners_out'][0] - NC.corners_of((0.4 * 0.2 / 1.3, 0.0, 3.0, 1, 1, 1, 0))).max() < 1e-6


def test_one_view_is_a_byte_copy():
    c, w = ens([NC.draw_object(np.random.RandomState(1))], [0.7])
    assert w['anchor'][0] == 0 and w['n_votes'][0] == 0 and w['agreement'][0] == 0 and w['min_iou'][0] == 0 and not w['fused']
    assert w['label_out'].tobytes() == c.labels[0].tobytes() and w['corners_out'].tobytes() == c.corners0().tobytes()


def test_a_quarter_turn_with_l_and_w_exchanged_is_the_same_box():
    a = (0, 0, 3, 2, 1, 1, 0.3)
    c, w = ens([a, EC.turned(a), a], [0.5, 0.5, 0.5])
    assert abs(w['agreement'][0] - 1) < 1e-6 and w['anchor'][0] == 0 and w['n_votes'][0] == 2
    assert np.abs(w['label_out'][0] - c.labels[0, 0]).max() < 1e-6           # a naive mean would give l = w = 5/3


def test_identical_views_tie_exactly_and_an_outlying_view_0_is_not_the_anchor():
    cs = EC.hand_cases()
    for metric in NC.METRICS:
        w = cs['identical'].expected(metric, 0.5)
        assert (w['anchor'] == 0).all() and (w['n_votes'] == 4).all()
        assert np.abs(w['agreement'] - 1).max() < 1e-6 and np.abs(w['min_iou'] - 1).max() < 1e-6
        assert np.abs(w['label_out'] - cs['identical'].labels[0]).max() < 1e-6
        w = cs['outlier0'].expected(metric, 0.5)
        assert (w['anchor'] > 0).all() and (w['n_votes'] >= 2).all()
        # the fused box sits on the three tight views, not on view 0
        tight = w['views'][1:, :, 3:6].astype(np.float64).mean(0)
        assert np.abs(w['label_out'][:, 3:6] - tight).max() < 0.05 < np.abs(w['views'][0, :, 3:6] - tight).max()


def test_a_vote_threshold_above_the_overlap_and_weights_that_count_as_zero():
    views = [NC.unit_cube(0.0), NC.unit_cube(0.2)]
    c, w = ens(views, [0.9, 0.6], vote=0.7)
    assert w['n_votes'][0] == 0 and w['label_out'].tobytes() == c.labels[0].tobytes() and w['corners_out'].tobytes() == c.corners0().tobytes()
    assert abs(w['agreement'][0] - 2 / 3) < 1e-6                              # the agreement does not depend on who votes
    for bad in (np.nan, -1.0, np.inf, -np.inf, 0.0):
        c, w = ens(views, [bad, 0.6])                                           # a bad anchor weight: the mean of the voters
        assert w['n_votes'][0] == 1 and abs(w['label_out'][0][3] - 0.2) < 1e-6
        c, w = ens(views, [bad, bad])                                           # W = 0: byte copies, the voter still counted
        assert w['n_votes'][0] == 1 and w['label_out'].tobytes() == c.labels[0].tobytes() and not w['fused']


def test_non_finite_labels_and_angles():
    c = EC.hand_cases()['non_finite']
    w = c.expected('3d', 0.0)
    assert list(w['anchor']) == [-1, 1, 0, 0] and list(w['n_votes']) == [0, 0, 1, 1]
    assert w['agreement'][0] == 0 and w['agreement'][1] == 0 and w['agreement'][2] > 0.9
    k0 = c.corners0()
    assert all(w['label_out'][i].tobytes() == c.labels[0, i].tobytes() and w['corners_out'][i].tobytes() == k0[i].tobytes() for i in (0,))
    assert w['label_out'][1].tobytes() == c.labels[1, 1].tobytes()             # the only valid view, unmirrored: its label
    assert np.array_equal(w['corners_out'][1], FE.label_corners(c.labels[1, 1]))
    # detection 3: its mirrored view 2 has a NaN angle and is not valid; the other two fuse
    assert sorted(w['ious'][3]) == [(0, 1)] and np.isfinite(w['label_out'][3]).all()


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------
def test_mirror_pin():
    """An independent definition: the corners of the un-mirrored label are, as a set, the corners of the input box reflected corner by
    corner -- turned by a into the centre view, x negated, turned back."""
    r = np.random.RandomState(3)
    worst = 0.0
    for _ in range(200):
        box, a = NC.draw_object(r), r.uniform(-np.pi, np.pi)
        label = FC.label_of(box)
        k = FE.label_corners(label).astype(np.float64)
        c, s = np.cos(np.float32(a).astype(np.float64)), np.sin(np.float32(a).astype(np.float64))
        xc, zc = k[:, 0] * c - k[:, 2] * s, k[:, 0] * s + k[:, 2] * c          # the way t3d_batch_assemble turns a point
        xc = -xc
        want = np.stack([xc * c + zc * s, k[:, 1], -xc * s + zc * c], 1)
        got = FE.label_corners(FE.unmirror(label, np.float32(a))).astype(np.float64)
        worst = max(worst, CC.corner_set_distance(got, want))
        assert -np.pi < FE.unmirror(label, np.float32(a))[6] <= np.float32(np.pi)
        back = FE.unmirror(FE.unmirror(label, np.float32(a)), np.float32(a))   # twice: the box itself (the heading modulo 2 pi)
        assert np.abs(back[:6] - label[:6]).max() < 1e-5 and abs(FF.wrap(float(back[6]) - float(label[6]))) < 1e-5
    assert worst < 1e-5, worst
    assert np.array_equal(FE.view_labels(np.zeros((2, 3, 7), np.float32), 0), np.zeros((2, 3, 7), np.float32))


# ---- the generated cases: their conditions, and DeviceEnsemble through the specification library ---------------------------------------
@pytest.mark.parametrize('metric,vote', EC.PASSES)
def test_generated_cases_keep_their_margins(metric, vote):
    """What the GPU tests rely on, on the seeds they use: the cap on redraws holds (asserted while the cases are built), no detection
    breaks a condition, and every pass fuses, leaves alone, anchors off view 0 and meets invalid views."""
    cs = EC.cases(metric, vote)
    gen = [c for c in cs.values() if not c.hand_built]
    assert sum(c.redrawn for c in gen) <= NC.MAX_REDRAWN * sum(c.n for c in gen)
    assert {c.n for c in gen} >= {1, 63, 64, 65, 257} and {c.V for c in gen} >= {1, 2, 3, 5, 8}
    assert {c.V * (c.V - 1) // 2 for c in gen} >= {0, 1, 3, 10, 28}
    assert {'far_45m', 'identical', 'outlier0', 'non_finite'} <= set(cs)
    assert np.abs(cs['far_45m'].labels[0, :, [3, 5]]).max() > 40
    fused = copies = off0 = invalid = 0
    for name, c in cs.items():
        assert not c.bad(metric, vote), name
        w = EC.expected_of(name, metric, vote)
        fused, copies = fused + len(w['fused']), copies + int(((w['anchor'] <= 0) & (w['n_votes'] == 0)).sum())
        off0, invalid = off0 + int((w['anchor'] > 0).sum()), invalid + int((~np.isfinite(c.labels).all(2)).sum())
        assert (w['agreement'] >= w['min_iou']).all() and (w['n_votes'] < max(c.V, 1)).all()
    assert fused > 200 and copies > 60 and off0 > 100 and invalid > 20
    bad = np.concatenate([c.weights.reshape(-1) for c in gen])
    assert (bad == 0).any() and (bad < 0).any() and np.isnan(bad).any() and np.isinf(bad).any()
    if vote > 0:                                        # the threshold turns some views away
        low = sum(int(EC.cases(metric, 0.0)[k].expected(metric, 0.0)['n_votes'].sum()) for k in ('n63_v2', 'n64_v3'))
        assert 0 < sum(int(EC.expected_of(k, metric, vote)['n_votes'].sum()) for k in ('n63_v2', 'n64_v3')) < low


@pytest.mark.parametrize('metric,vote', [('3d', 0.0), ('bev', 0.5)])
def test_device_ensemble_on_the_specification_library(metric, vote):
    rt = cpu_rt()
    for name, c in EC.cases(metric, vote).items():
        EC.check_case(rt, name, metric, vote)
        got, want = EC.run_case(rt, c, metric, vote), EC.expected_of(name, metric, vote)
        assert all(got[k].tobytes() == want[k].tobytes() for k in FE.OUTPUTS), name
    for name in ('n64_v3', 'n63_v2', 'n1_v8'):
        got, want = EC.moved(rt, name, metric, vote), EC.expected_of(name, metric, vote)
        assert all(got[k].tobytes() == want[k].tobytes() for k in FE.OUTPUTS), name + ' moved'
    c = EC.cases(metric, vote)['n64_v3']
    got = EC.run(rt, c.labels[:, :0], c.weights[:, :0], np.zeros((0, 8, 3), np.float32), c.flip_mask, None, vote, metric)
    assert all(len(got[k]) == 0 for k in FE.OUTPUTS)


# ---- the argument struct ---------------------------------------------------------------------------------------------------------------
def test_struct_follows_the_header_and_the_compiler(tmp_path):
    assert abi.ENTRY_POINTS['t3d_detect_ensemble'][0]._type_ is abi.DetectEnsembleArgs
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\}\s*t3d_detect_ensemble_args;', h).group(1), flags=re.S)
    names = [re.findall(r'(\w+)\s*(?:\[\w+\])?\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]
    assert names == [f[0] for f in abi.DetectEnsembleArgs._fields_]
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "t3d.h"\nint main(void) { printf("%zu %d %llu %llu %llu %zu %zu %d %d\\n", '
                   'sizeof(t3d_detect_ensemble_args), T3D_V2_SIZE_detect_ensemble_args, (unsigned long long)T3D_DETECT_ENSEMBLE_WORKSPACE_BYTES(1001, 8), '
                   '(unsigned long long)T3D_DETECT_ENSEMBLE_WORKSPACE_BYTES(1001, 3), (unsigned long long)T3D_DETECT_ENSEMBLE_WORKSPACE_BYTES(7, 1), '
                   'offsetof(t3d_detect_ensemble_args, flip_mask), offsetof(t3d_detect_ensemble_args, n_votes), T3D_DETECT_ENSEMBLE_MAX_VIEWS, '
                   'T3D_ABI_VERSION); return 0; }\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'size')])
    size, v2, ws8, ws3, ws1, off_f, off_v, views, version = (int(v) for v in subprocess.check_output([str(tmp_path / 'size')], text=True).split())
    assert size == v2 == C.sizeof(abi.DetectEnsembleArgs) == 232 and abi.DetectEnsembleArgs().struct_size == size and version == 3
    assert views == abi.DETECT_ENSEMBLE_MAX_VIEWS == EN.MAX_VIEWS == 8
    assert ws8 == abi.detect_ensemble_workspace_bytes(1001, 8) == 1001 * 28 * 4 and ws3 == abi.detect_ensemble_workspace_bytes(1001, 3) == 12016
    assert ws1 == abi.detect_ensemble_workspace_bytes(7, 1) == 0
    assert off_f == abi.DetectEnsembleArgs.flip_mask.offset and off_v == abi.DetectEnsembleArgs.n_votes.offset


def full_args(buf, **kw):
    f, i = C.cast(buf, abi.F), C.cast(buf, abi.I)
    a = abi.DetectEnsembleArgs(n=10, V=3, metric=0, flip_mask=0b010, vote_threshold=0.25, rot_angle=f, corners0=f, workspace=C.addressof(buf),
                               workspace_bytes=abi.detect_ensemble_workspace_bytes(10, 3), label_out=f, corners_out=f, agreement=f, min_iou=f,
                               anchor=i, n_votes=i)
    for v in range(3):
        a.label[v], a.weight[v] = f, f
    for k, v in kw.items():
        if k in ('label', 'weight'):
            getattr(a, k)[v] = None
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize('which', ['built', 'specification'])
def test_the_library_checks_before_it_launches(which):
    """No GPU needed: the struct size, the number of views, the metric, the mirror mask, the vote threshold, the pointers and the
    workspace are checked before anything is launched -- by the built library and, with the same answers, by the specification library."""
    lib, null = (abi.load() if which == 'built' else SpecLib()), C.c_void_p(0)
    call = lambda a: lib.t3d_detect_ensemble(C.byref(a), null)
    a = abi.DetectEnsembleArgs()
    a.struct_size -= 8
    assert call(a) == abi.ERR_ABI
    assert call(abi.DetectEnsembleArgs()) == -1                              # V == 0
    assert call(abi.DetectEnsembleArgs(V=1)) == 0 and call(abi.DetectEnsembleArgs(V=8, flip_mask=0b10101010)) == 0      # n == 0: nothing to do
    assert call(abi.DetectEnsembleArgs(n=4, V=9, metric=0, vote_threshold=0.5)) == -2      # T3D_ERR_SHAPE
    assert call(abi.DetectEnsembleArgs(n=4, V=3, metric=0, vote_threshold=0.5)) == -1      # null pointers
    buf = (C.c_uint64 * 64)()
    for bad in (dict(metric=2), dict(metric=-1), dict(vote_threshold=-0.01), dict(vote_threshold=1.01), dict(vote_threshold=float('nan')),
                dict(n=-1), dict(V=0), dict(V=-1), dict(flip_mask=0b011), dict(flip_mask=0b1010), dict(flip_mask=1 << 31),
                dict(workspace_bytes=abi.detect_ensemble_workspace_bytes(10, 3) - 8), dict(workspace=C.addressof(buf) + 4), dict(workspace=None)):
        assert call(full_args(buf, **bad)) == -1, bad
    for k in ('corners0', 'label_out', 'corners_out', 'agreement', 'min_iou', 'anchor', 'n_votes'):
        assert call(full_args(buf, **{k: None})) == -1, k
    for v in range(3):
        assert call(full_args(buf, label=v)) == -1 and call(full_args(buf, weight=v)) == -1, v
    assert call(full_args(buf, n=0, corners0=None, workspace=None)) == 0


def test_nine_views_are_refused_through_device_ensemble():
    import torch
    rt = cpu_rt()
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(abi.T3DError, match='T3D_ERR_SHAPE'):
        EN.DeviceEnsemble(rt).run([z(2, 7)] * 9, [z(2)] * 9, z(2, 24))


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def test_options_and_flag_errors(tmp_path):
    assert EN.check_options() == (None, False, None, None)
    assert EN.check_options(2) == (2, False, 0.0, None) and EN.check_options(8, True, 0.5, 0.25) == (8, True, 0.5, 0.25)
    assert EN.check_options(3, False, 0, 1) == (3, False, 0.0, 1.0)
    for bad in ((1,), (9,), (0,), (2.5,), (None, True), (None, False, 0.5), (None, False, None, 0.5), (3, False, -0.1), (3, False, 1.1),
                (3, False, float('nan')), (3, False, None, 1.5), (3, False, None, float('nan'))):
        with pytest.raises(ValueError):
            EN.check_options(*bad)
    views = EN.views_of(5, True, seed=3)
    assert views[0] == (3, False) and [f for _, f in views] == [False, True, False, True, False] and len({s for s, _ in views}) == 5
    assert [f for _, f in EN.views_of(4, False, seed=3)] == [False] * 4 and EN.views_of(4, False, 3)[1][0] == views[1][0]
    assert EN.flip_mask_of(views) == 0b01010 and EN.EnsembleRequest(views).flip_mask == 0b01010
    assert EN.views_of(3, seed=4)[1][0] != views[1][0]                       # the further seeds follow the run's
    for bad in ([(1, True)], [(1, False)] * 9, []):
        with pytest.raises(ValueError):
            EN.EnsembleRequest(bad)
    for kw in (dict(tta=1), dict(tta=9), dict(tta_flip=True), dict(tta_vote_iou=0.5), dict(min_view_iou=0.5), dict(tta=3, min_view_iou=1.5)):
        with pytest.raises(ValueError):
            DT.Detector(object(), **kw)
    needed = ['--dataset_dir', str(tmp_path), '--idx_path', 'none', '--rgb_detection_path', 'none']
    for extra in (['--tta', '1'], ['--tta', '9'], ['--tta_flip'], ['--tta_vote_iou', '0.5'], ['--min_view_iou', '0.5'],
                  ['--tta', '3', '--min_view_iou', '1.5'], ['--tta', '3', '--tta_vote_iou', '-1'], ['--tta', '3', '--sweep', '--sweep_nms_iou', '0.25'],
                  ['--tta', 'x']):
        with pytest.raises(SystemExit):
            DT.main(needed + extra, log=lambda *a: None)
    base = ['--idx_path', 'x', '--classes', 'table', '--out_dir', 'o']
    for extra in (['--tta', '1'], ['--tta_flip'], ['--min_view_iou', '0.3'], ['--tta', '2', '--min_view_iou', '2']):
        with pytest.raises(SystemExit):
            AL.parse(base + extra)
    args, _ = AL.parse(base + ['--tta', '4', '--tta_flip', '--min_view_iou', '0.3'])
    assert (args.tta, args.tta_flip, args.tta_vote_iou, args.min_view_iou) == (4, True, None, 0.3)
    with pytest.raises((SystemExit, ValueError)):                            # not in this command
        SI.build_flags(['--device_decode', '--from_rgb_detection', '--tta', '3'])
    with pytest.raises(ValueError):
        SI.inference(None, None, None, None, 4, decode='host', views=EN.EnsembleRequest(views))


# ---- the flow --------------------------------------------------------------------------------------------------------------------------
def test_without_tta_the_result_files_are_those_of_the_two_step_route(tmp_path):
    """No new flag: `detect` writes, byte for byte, what sunrgbd_data + semisup_infer --device_decode write -- a route that reads none of
    the new options -- and what the records of a plain Detector print."""
    rt, quiet = cpu_rt(), (lambda *a: None)
    ids, folder, idx, dets = DC.write_data_set(tmp_path)
    res = os.path.join(str(tmp_path), 'plain')
    pred = DT.main(['--dataset_dir', str(tmp_path), '--idx_path', idx, '--rgb_detection_path', folder, '--result_dir', res] + DC.MODEL_FLAGS, rt=rt, log=quiet)
    got = DC.read_results(res)
    two, _, _ = DC.two_step(rt, tmp_path, ids, folder, 'two_step', True)
    assert got == two
    d = pred.decoded
    assert all(getattr(d, k) is None for k in ('view_label', 'view_score', 'view_iou', 'view_min_iou', 'anchor_view', 'n_views_voted', 'accept'))
    records = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt).detect(DC.load_scenes(tmp_path, ids), dets, scene_ids=ids)
    lines = DC.record_lines(ids, records)
    assert all(lines.get(c, '') == t for c, t in got.items()) and set(lines) <= set(got)


def test_detect_with_views_end_to_end(tmp_path):
    rt, quiet = cpu_rt(), (lambda *a: None)
    report, d, s = EC.check_flow(rt, tmp_path, exact=True)
    print('\n'.join(report))
    ids, scenes, dets, want, n = s['ids'], s['scenes'], s['dets'], s['want'], len(d)
    flags = lambda: TS.build_flags(DC.MODEL_FLAGS)
    # the records are the specification applied to view_label and view_score
    records = DT.Detector(flags(), rt=rt, tta=3, tta_flip=True).detect(scenes, dets, scene_ids=ids)
    flat = [r for recs in records for r in recs]
    assert len(flat) == n
    for i, (r, r0) in enumerate(zip(flat, s['plain'])):
        assert set(r) == set(r0) | {'view_iou', 'view_min_iou', 'views_voted', 'anchor_view'}
        assert np.array_equal(r['label'], want['label_out'][i].astype(np.float64)) and np.array_equal(r['corners'], want['corners_out'][i].astype(np.float64))
        assert r['view_iou'] == float(want['agreement'][i]) and r['view_min_iou'] == float(want['min_iou'][i])
        assert r['views_voted'] == want['n_votes'][i] and r['anchor_view'] == want['anchor'][i]
        assert all(np.array_equal(r[k], r0[k]) for k in ('class', 'box2d', 'prob', 'score'))
    # the command: the result files are the records
    base = ['--dataset_dir', str(tmp_path), '--idx_path', s['idx'], '--rgb_detection_path', s['folder']] + DC.MODEL_FLAGS
    res = lambda name: os.path.join(str(tmp_path), name)
    logged = []
    pred = DT.main(base + ['--result_dir', res('tta'), '--tta', '3', '--tta_flip'], rt=rt, log=logged.append)
    lines = DC.record_lines(ids, records)
    got = DC.read_results(res('tta'))
    assert all(lines.get(c, '') == t for c, t in got.items()) and set(lines) <= set(got)
    assert any(l.startswith('tta: 3 views (1 mirrored), fused ') for l in logged) and np.array_equal(pred.decoded.view_iou, d.view_iou)
    # min_view_iou drops exactly the detections below it
    values = np.sort(d.view_iou)
    A = float((values[n // 2 - 1] + values[n // 2]) / 2.0)
    assert values[n // 2 - 1] < A < values[n // 2]
    logged = []
    kept = DT.Detector(flags(), rt=rt, tta=3, tta_flip=True, min_view_iou=A, log=logged.append).detect(scenes, dets, scene_ids=ids)
    flat_kept = [r for recs in kept for r in recs]
    assert [r['view_iou'] for r in flat_kept] == [r['view_iou'] for r in flat if r['view_iou'] >= A] and 0 < len(flat_kept) == n - n // 2 < n
    assert all(np.array_equal(a['label'], b['label']) for a, b in zip(flat_kept, [r for r in flat if r['view_iou'] >= A]))
    assert logged[0] == 'consistency: kept %d of %d (view_iou < %g: %d)' % (len(flat_kept), n, A, n // 2), logged
    # ... with the consistency measures and a fusion behind it
    both = DT.Detector(flags(), rt=rt, tta=3, tta_flip=True, min_view_iou=A, consistency=True, nms_iou=0.25, nms_fuse=True).detect(
        CC.scenes_with_sizes(tmp_path, ids), dets, scene_ids=ids)
    assert all({'view_iou', 'reproj_iou', 'votes'} <= set(r) and r['view_iou'] >= A for recs in both for r in recs)
    DT.main(base + ['--result_dir', res('tta_min'), '--tta', '3', '--tta_flip', '--min_view_iou', repr(A), '--consistency',
                    '--consistency_json', res('rows.json')], rt=rt, log=quiet)
    import json
    rows = json.load(open(res('rows.json')))
    assert len(rows) == n and [r['accepted'] for r in rows] == [bool(v >= A) for v in d.view_iou] and all('anchor_view' in r for r in rows)
    assert DC.read_results(res('tta_min')) == {c: t for c, t in {**{c: '' for c in got}, **DC.record_lines(ids, kept)}.items()}


def test_a_detection_rejected_by_min_view_iou_suppresses_nothing(tmp_path):
    """One object reported twice: the box whose views agree less is given the better rank.  With NMS alone it suppresses the other; with
    min_view_iou between the two values it is rejected before the groups are built, and the other survives."""
    rt = cpu_rt()
    ids, folder, idx, dets = DC.write_data_set(tmp_path)
    scenes = DC.load_scenes(tmp_path, ids)[:1]
    name, box, _ = next(x for x in dets[0] if x != DC.SPARSE)
    pair = [tuple(box), tuple(np.asarray(box) + (6.0, 4.0, 6.0, 4.0))]
    run = lambda probs, **kw: DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, tta=2, **kw).detect(
        scenes, [[(name, pair[0], probs[0]), (name, pair[1], probs[1])]], scene_ids=ids[:1])[0]
    both = run((0.9, 0.8))
    v = [r['view_iou'] for r in both]
    assert len(both) == 2 and v[0] != v[1], v
    worse = int(v[1] < v[0])
    probs = (0.9, 0.8) if worse == 0 else (0.8, 0.9)
    A = (v[0] + v[1]) / 2.0
    alone = run(probs, nms_iou=0.05)
    assert len(alone) == 1 and alone[0]['prob'] == 0.9 and np.array_equal(alone[0]['box2d'], pair[worse])
    lines = []
    kept = run(probs, nms_iou=0.05, min_view_iou=A, log=lines.append)
    assert len(kept) == 1 and kept[0]['prob'] == 0.8 and np.array_equal(kept[0]['box2d'], pair[1 - worse])
    assert kept[0]['view_iou'] == v[1 - worse] >= A > v[worse]
    assert lines[0] == 'consistency: kept 1 of 2 (view_iou < %g: 1)' % A and 'kept 1 of 1' in lines[-1], lines


def test_autolabel_writes_only_the_boxes_whose_views_agree(tmp_path):
    rt, quiet = cpu_rt(), (lambda *a: None)
    ids, folder, idx, dets = DC.write_data_set(tmp_path)
    classes = sorted(set(x[0] for scene in dets for x in scene))
    base = ['--dataset_dir', str(tmp_path), '--idx_path', idx, '--classes'] + classes
    first = AL.main(base + ['--out_dir', str(tmp_path / 'auto0'), '--tta', '3', '--tta_flip'] + DC.MODEL_FLAGS, rt=rt, log=quiet)
    values = sorted(r['view_iou'] for r in first['_records'] if r['detected'])
    assert all(r['accepted'] for r in first['_records'] if r['detected']) and first['tta'] == dict(views=3, flip=True, vote_iou=0.0, min_view_iou=None)
    A = (values[len(values) // 2 - 1] + values[len(values) // 2]) / 2.0
    lines = []
    s = AL.main(base + ['--out_dir', str(tmp_path / 'auto'), '--tta', '3', '--tta_flip', '--min_view_iou', repr(A), '--score_against_labels']
                + DC.MODEL_FLAGS, rt=rt, log=lines.append)
    records = [r for r in s['_records'] if r['detected']]
    assert [r['accepted'] for r in records] == [r['view_iou'] >= A for r in records] and 0 < sum(r['accepted'] for r in records) < len(records)
    assert [r['view_iou'] for r in records] == [r['view_iou'] for r in first['_records'] if r['detected']]
    assert sum(c['rejected_by']['min_view_iou'] for c in s['classes'].values()) == sum(not r['accepted'] for r in records)
    written = sum(len([l for l in open(tmp_path / 'auto' / 'training' / 'label_dimension' / f) if l.strip()])
                  for f in os.listdir(tmp_path / 'auto' / 'training' / 'label_dimension'))
    assert written == sum(r['accepted'] for r in records)
    by = s['score_against_labels']
    assert sum(v['min_view_iou']['accepted']['n'] for v in by.values()) == written
    assert sum(v['min_view_iou']['rejected']['n'] for v in by.values()) == len(records) - written
    assert any('by --min_view_iou' in l for l in lines)
    plain = AL.main(base + ['--out_dir', str(tmp_path / 'auto1')] + DC.MODEL_FLAGS, rt=rt, log=quiet)      # without the flags: as it was
    assert 'tta' not in plain and all('view_iou' not in r for r in plain['_records'])


def test_vis_dir_draws_the_fused_boxes_and_says_how_the_views_agreed(tmp_path):
    """--vis_dir with --tta: the legend entries gain the four view fields, the result files are those of the run without pictures, and
    t3d_render is handed the corners t3d_detect_ensemble wrote."""
    import json
    seen = []

    class VisLib(SpecLib):
        def t3d_render(self, a, stream):
            p = a._obj
            seen.append(np.ctypeslib.as_array(p.corners, shape=(p.n_corner_boxes, 8, 3)).copy())
            return super().t3d_render(a, stream)

    rt, quiet = Runtime(device='cpu', lib=VisLib()), (lambda *a: None)
    ids, folder, idx, dets = DC.write_data_set(tmp_path)
    base = ['--dataset_dir', str(tmp_path), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS + ['--tta', '2', '--tta_flip']
    res = lambda name: os.path.join(str(tmp_path), name)
    DT.main(base + ['--result_dir', res('tta')], rt=rt, log=quiet)
    assert not seen
    DT.main(base + ['--result_dir', res('tta_vis'), '--vis_dir', res('pics')], rt=rt, log=quiet)
    assert DC.read_results(res('tta_vis')) == DC.read_results(res('tta'))
    det = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, tta=2, tta_flip=True)
    meta, d = det.decode_all([det.extract(DC.load_scenes(tmp_path, ids), dets, ids)])
    assert seen and all(np.array_equal(k[:len(d)], d.corners.astype(np.float32)) for k in seen)
    assert not np.array_equal(d.corners, FE.ensemble(d.view_label[:1].astype(np.float32), np.ones((1, len(d)), np.float32))['corners_out'])
    fields = []
    for s in ids:
        legend = json.load(open(os.path.join(res('pics'), '%06d.json' % s)))
        fields += [(b['view_iou'], b['view_min_iou'], b['views_voted'], b['anchor_view']) for b in legend['boxes'] if b['kind'] == 'kept']
    assert fields == [(float(a), float(b), int(c), int(e)) for a, b, c, e in zip(d.view_iou, d.view_min_iou, d.n_views_voted, d.anchor_view)]
