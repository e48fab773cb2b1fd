"""CPU: the visibility stage through the NumPy specification (tests/fake_visibility.py): the constructed one-wall scenes against counts
written by hand, the options and their errors, the request, the stage's place among the stages behind the decode and its accept rule,
the fields it adds to records and reports, and what the measure and the slide do on clean label boxes.  That the records of a run
WITHOUT the flags are byte for byte what they were is shown by the existing transcript tests, which this change leaves as they are;
here a plain run is compared with a run that only measures, field by field as bytes.  tests/visibility_check.py's kernel checks run here
through the specification too, so that the checkers themselves are exercised without a device."""
import json

import numpy as np
import pytest

import detect_check as DC
import fake_consistency as FK
import fake_floor as FF
import fake_fuse as FU
import fake_nms as FN
import fake_visibility as FV
import scene_check as SK
import stages_check as SC
import visibility_check as VC
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from transferable3d_amd import abi, detect as DT, semisup_infer as SI, sunrgbd_data as SD, synth_scenes as SS, test_semisup as TS, visibility as VS
from transferable3d_amd.engine import Runtime


class SpecLib(FV.VisibilitySpec, FF.FloorSpec, FK.ConsistencySpec, FU.DetectFuseSpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib, FF.FakeSceneLib):
    pass


@pytest.fixture(scope='module')
def rt():
    return Runtime(device='cpu', lib=SpecLib())


def flags():
    return TS.build_flags(DC.MODEL_FLAGS)


# ---- the two entry points ------------------------------------------------------------------------------------------------------------------
def test_the_specification_counts_what_was_counted_by_hand(rt):
    """visibility_check.hand_cases and case_constructed state the geometry and the counts."""
    VC.check_hand_cases(rt)
    VC.check_range_constructed(rt)


def test_the_kernel_checks_hold_for_the_specification(rt):
    for S in (1, 3):
        for ld in (3, 6):
            VC.check_range_batch(rt, S, ld)
    VC.check_range_flags(rt)
    VC.check_range_batch_independence(rt)
    VC.check_scene_range_refusals(rt.lib)
    VC.check_detect_visibility_refusals(rt.lib)
    VC.check_detect_batch_independence(rt)
    for n in VC.DETECT_SIZES:
        for K in (1, 3, 9):
            for mode in (0, 1):
                VC.check_detect_visibility(rt, n, K, mode)


def test_the_library_refuses_what_the_specification_refuses():
    """No device needed: a refusal comes before any launch."""
    lib = abi.load()
    VC.check_scene_range_refusals(lib)
    VC.check_detect_visibility_refusals(lib)


def test_the_structs_are_the_headers():
    import ctypes as C
    const = SK_const()
    for cname, cls in (('scene_range_args', abi.SceneRangeArgs), ('detect_visibility_args', abi.DetectVisibilityArgs)):
        assert const['sizeof_' + cname] == const['T3D_V2_SIZE_' + cname] == C.sizeof(cls), cname
    assert (const['T3D_RANGE_EMPTY'], const['T3D_RANGE_BLOCKS'], const['T3D_RANGE_MAX_CELLS']) == (abi.RANGE_EMPTY, abi.RANGE_BLOCKS, abi.RANGE_MAX_CELLS)
    assert (const['T3D_RANGE_NO_CALIB'], const['T3D_RANGE_BAD_GRID'], const['T3D_VIS_MAX_OFFSETS']) == (abi.RANGE_NO_CALIB, abi.RANGE_BAD_GRID, abi.VIS_MAX_OFFSETS)
    assert tuple(const['T3D_VIS_' + k] for k in ('NO_SCENE', 'NOT_FINITE', 'BEHIND', 'NO_RAYS', 'NO_EVIDENCE', 'SNAPPED')) == (
        abi.VIS_NO_SCENE, abi.VIS_NOT_FINITE, abi.VIS_BEHIND, abi.VIS_NO_RAYS, abi.VIS_NO_EVIDENCE, abi.VIS_SNAPPED)
    assert C.sizeof(abi.DetectVisibilityArgs) - abi.DetectVisibilityArgs.offsets.offset == 8 * abi.VIS_MAX_OFFSETS + 6 * 8
    assert 't3d_scene_range' in abi.ENTRY_POINTS and abi.ENTRY_POINTS['t3d_detect_visibility'][0]._type_ is abi.DetectVisibilityArgs


def SK_const():
    """The header's constants and sizes, through a C compiler."""
    import os
    import subprocess
    import tempfile
    names = ['T3D_V2_SIZE_scene_range_args', 'T3D_V2_SIZE_detect_visibility_args', 'T3D_RANGE_EMPTY', 'T3D_RANGE_BLOCKS', 'T3D_RANGE_MAX_CELLS',
             'T3D_RANGE_NO_CALIB', 'T3D_RANGE_BAD_GRID', 'T3D_VIS_MAX_OFFSETS'] + ['T3D_VIS_' + k for k in ('NO_SCENE', 'NOT_FINITE', 'BEHIND', 'NO_RAYS', 'NO_EVIDENCE', 'SNAPPED')]
    src = '#include <stdio.h>\n#include "t3d.h"\nint main(){' + ''.join('printf("%s %%lld\\n",(long long)%s);' % (n, n) for n in names) + \
        'printf("sizeof_scene_range_args %lld\\n",(long long)sizeof(t3d_scene_range_args));' \
        'printf("sizeof_detect_visibility_args %lld\\n",(long long)sizeof(t3d_detect_visibility_args));return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'c.c')
        open(path, 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(SK.ROOT, 'include'), path, '-o', os.path.join(tmp, 'c')])
        out = subprocess.check_output([os.path.join(tmp, 'c')]).decode()
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


# ---- options, flags, the request ---------------------------------------------------------------------------------------------------------
def test_options_are_checked():
    o = VS.VisibilityOptions()
    assert (o.cell, o.margin, o.min_chord, o.min_rays) == (4, 0.05, 0.1, 16)
    for kw in (dict(cell=0), dict(cell=2.5), dict(cell=2000), dict(margin=-0.1), dict(margin=float('nan')), dict(min_chord=float('inf')), dict(min_chord=-1.0),
               dict(min_rays=-1), dict(min_rays=1.5)):
        with pytest.raises(ValueError):
            VS.VisibilityOptions(**kw)
    v = VS.check_options()
    assert not v.on and v.max_see_through is None
    assert VS.check_options(visibility=True).on and VS.check_options(max_see_through=0.0).on and VS.check_options(max_see_through=1.0).max_see_through == 1.0
    v = VS.check_options(max_see_through=0.5, visibility_cell=8, visibility_margin=0.1, visibility_min_chord=0.0, visibility_min_rays=4)
    assert (v.max_see_through, v.options.cell, v.options.margin, v.options.min_chord, v.options.min_rays) == (0.5, 8, 0.1, 0.0, 4)
    for kw in (dict(visibility_cell=4), dict(visibility_margin=0.05), dict(visibility_min_chord=0.1), dict(visibility_min_rays=16),
               dict(visibility=True, visibility_min_rays=16), dict(max_see_through=-0.1), dict(max_see_through=1.5), dict(max_see_through=float('nan')),
               dict(visibility=True, visibility_cell=0), dict(visibility=True, visibility_margin=-1.0)):
        with pytest.raises(ValueError):
            VS.check_options(**kw)
    for kw in (dict(visibility_cell=4), dict(max_see_through=2.0), dict(visibility_min_rays=3)):          # Detector checks them before it builds a model
        with pytest.raises(ValueError):
            DT.Detector(object(), **kw)
    assert set(VS.FLAGS) <= set(DT.STAGE_KEYWORDS) and 'visibility' in DT.RECORD_GROUPS and 'visibility' in DT.ROW_GROUPS
    assert VS.scene_size({'K': [[40.3, 0, 33.3], [0, 39.6, 17.2], [0, 0, 1]]}) == (67, 35) and VS.scene_size({'K': np.eye(3), 'image_wh': (27, 19)}) == (27, 19)
    dims, goff = VS.grids_of([(27, 19), (730, 530)], 4)
    assert dims.tolist() == [[7, 5], [183, 133]] and goff.tolist() == [0, 35, 35 + 183 * 133]


BASE = ['--idx_path', 'none', '--rgb_detection_path', 'none']


@pytest.mark.parametrize('argv,message', [
    (['--visibility_cell', '4'], 'needs --visibility'), (['--visibility_margin', '0.1'], 'needs --visibility'), (['--visibility_min_chord', '0.1'], 'needs --visibility'),
    (['--visibility', '--visibility_min_rays', '8'], 'needs --max_see_through'), (['--max_see_through', '1.5'], 'must lie in [0, 1]'),
    (['--max_see_through', 'nan'], 'must lie in [0, 1]'), (['--visibility', '--visibility_cell', '0'], 'visibility_cell'),
    (['--visibility', '--visibility_margin', 'nan'], 'visibility_margin'), (['--visibility', '--sweep'], 'does not go with --visibility'),
    (['--sweep', '--max_see_through', '0.5'], 'does not go with --max_see_through'), (['--rescore_fit', 'm.json', '--visibility'], 'does not go with --visibility'),
    (['--rescore_fit', 'm.json', '--max_see_through', '0.5'], 'does not go with --max_see_through')])
def test_flag_errors_are_argument_errors(argv, message, capsys):
    with pytest.raises(SystemExit):
        DT.main(BASE + argv + DC.MODEL_FLAGS)
    assert message in capsys.readouterr().err


def test_autolabel_takes_the_flags(capsys):
    from transferable3d_amd import autolabel as AL
    base = ['--idx_path', 'none', '--classes', 'chair', '--out_dir', 'none']
    args, _ = AL.parse(base + ['--max_see_through', '0.5', '--visibility_min_rays', '8', '--visibility_cell', '8'] + DC.MODEL_FLAGS)
    assert args.max_see_through == 0.5 and args.visibility_min_rays == 8 and args.visibility_cell == 8 and not args.visibility
    with pytest.raises(SystemExit):
        AL.parse(base + ['--visibility_min_rays', '8'] + DC.MODEL_FLAGS)
    assert 'needs --max_see_through' in capsys.readouterr().err
    rec = lambda see, n, fl=0: {'class': 'chair', 'detected': True, 'accepted': True, 'see_through': see, 'visibility_evidence': n, 'visibility_flags': fl}
    records = [rec(0.9, 20), rec(0.9, 7), rec(0.4, 20), rec(1.0, 0, abi.VIS_NO_SCENE), rec(0.51, 8)]
    tests = SI.active_tests(VS.check_options(max_see_through=0.5, visibility_min_rays=8))
    c = AL.count(records, ['chair'], tests)['chair']
    assert c['rejected_by'] == {'max_see_through': 2} and AL.rejected_by(tests, records)['max_see_through'].tolist() == [True, False, False, False, True]


def test_semisup_infer_and_evaluate_do_not_take_the_flags(capsys):
    from transferable3d_amd import evaluate_sunrgbd as ES
    with pytest.raises(SystemExit):
        SI.build_flags(['--device_decode', '--visibility'] + DC.MODEL_FLAGS)
    with pytest.raises(SystemExit):
        ES.main(['--pred_dir', 'none', '--idx_path', 'none', '--max_see_through', '0.5'])
    assert 'unrecognized arguments: --max_see_through' in capsys.readouterr().err


def test_request_is_checked():
    calib, dims, goff, rng = np.zeros((2, 20)), np.zeros((2, 2), np.int32), np.zeros(3, np.int64), np.zeros(0, np.uint32)
    r = VS.VisibilityRequest(calib, dims, goff, rng, [0, 1, -1])
    assert len(r) == 3 and r.max_see_through is None and r.scene_index.dtype == np.int32 and r.options.cell == 4
    for bad in (lambda: VS.VisibilityRequest(calib, dims, goff, rng, [0, 2]), lambda: VS.VisibilityRequest(calib, dims, goff, rng, [-2]),
                lambda: VS.VisibilityRequest(calib, dims[:1], goff, rng, [0]), lambda: VS.VisibilityRequest(calib, dims, goff[:2], rng, [0]),
                lambda: VS.VisibilityRequest(calib, dims, goff, rng, [0], max_see_through=1.5)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="decode='device'"):
        SI.inference(None, None, None, None, 4, decode='host', visibility=r)
    with pytest.raises(ValueError, match='visibility request'):
        SI.DeviceStages(None, 4, 2, 16, visibility=r)


# ---- the stage among the stages ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def world(rt):
    """Four generated scenes whose detector reports every labelled object twice, a plain run and a run that only measures."""
    ss = SK.scene_set(rt, 4, det_dup=1.0, det_miss=0.0, det_confuse=0.0, det_fp_per_image=0.0)
    scenes = [{'points': s['depth'], 'Rtilt': s['Rtilt'], 'K': s['K']} for s in ss.scenes]
    dets = [s['detections'] for s in ss.scenes]
    plain = DT.Detector(flags(), rt=rt).detect(scenes, dets, scene_ids=ss.ids)
    det = DT.Detector(flags(), rt=rt, visibility=True)
    parts = [det.extract(scenes, dets, ss.ids)]
    meta, d = det.decode_all(parts)
    return dict(ss=ss, scenes=scenes, dets=dets, plain=plain, meta=meta, d=d, parts=parts, det=det)


def spec_of(world_, d, parts, o):
    part = parts[0]['range']
    return FV.detect_visibility(d.label.astype(np.float32), d.corners.astype(np.float32), [m.scene for m in world_['meta']], part['calib'], part['dims'],
                                part['offsets'], part['range'].numpy().view(np.uint32), o.cell, [0.0], o.margin, o.min_chord, 0, 0)


def test_measuring_adds_fields_and_changes_nothing_else(rt, world):
    records = DT.Detector(flags(), rt=rt, visibility=True).detect(world['scenes'], world['dets'], scene_ids=world['ss'].ids)
    n = 0
    for a, b in zip(world['plain'], records):
        assert len(a) == len(b)
        for r, q in zip(a, b):
            assert list(q)[:len(r)] == list(r) and list(q)[len(r):] == ['see_through', 'occluded', 'support', 'visibility_flags']
            assert all(np.asarray(r[k]).tobytes() == np.asarray(q[k]).tobytes() for k in r)
            n += 1
    d, part = world['d'], world['parts'][0]['range']
    assert n == len(d) >= 8 and d.accept is None and d.keep is None and 'range' not in DT.Detector(flags(), rt=rt).extract(world['scenes'], world['dets'], world['ss'].ids)
    # the part keeps the map the specification builds from the scenes' points, on grids of ceil(2 cx) x ceil(2 cy) pixels
    W, H = SK.W, SK.H
    assert part['dims'].tolist() == [[-(-W // 4), -(-H // 4)]] * 4 and len(part['range']) == part['offsets'][-1]
    points = np.concatenate([s['depth'] for s in world['ss'].scenes])
    offsets = np.concatenate([[0], np.cumsum([len(s['depth']) for s in world['ss'].scenes])])
    rng, counts = FV.scene_range_batch(points, offsets, part['calib'], np.arange(4), part['dims'], part['offsets'], len(part['range']), 4)
    assert VC.same(part['range'].numpy().view(np.uint32), rng) and VC.same(part['counts'], counts) and (counts[:, 2] > 0.5 * part['dims'].prod(1)).all()
    want = spec_of(world, d, world['parts'], world['det'].visibility.options)
    assert np.array_equal(d.visibility_profile, want[0][:, 0]) and VC.same(np.stack([d.see_through, d.occluded, d.support], 1), want[1])
    assert np.array_equal(d.visibility_flags, want[3]) and (d.visibility_profile[:, 0] > 0).sum() >= len(d) // 2
    fields = DT.fields_of(d, 0, DT.RECORD_GROUPS, as_lists=True)
    assert list(fields) == ['see_through', 'occluded', 'support', 'visibility_flags'] and fields['see_through'] == d.see_through[0]
    json.dumps(fields)


def test_a_rejected_box_is_in_no_group_and_the_floor_stage_runs_first(rt, world):
    d0, n = world['d'], len(world['d'])
    evidence = d0.visibility_profile[:, VS.THROUGH] + d0.visibility_profile[:, VS.INSIDE]
    enough = (evidence >= 4) & ((d0.visibility_flags & VS.UNMEASURED) == 0)
    values = np.unique(d0.see_through[enough])
    assert len(values) >= 2 and (~enough).any(), (values, evidence)
    F = float((values[-2] + values[-1]) / 2.0)
    lines = []
    det = DT.Detector(flags(), rt=rt, max_see_through=F, visibility_min_rays=4, floor=True, nms_iou=0.05, log=lines.append)
    parts = [det.extract(world['scenes'], world['dets'], world['ss'].ids)]
    with SC.Stages(rt) as cap:
        meta, d = det.decode_all(parts)
    batches = (n + 3) // 4
    assert cap.entry_points == ['decode'] * batches + ['floor', 'visibility', 'nms'], cap.entry_points
    assert VC.same(d.see_through, d0.see_through) and np.array_equal(d.visibility_flags, d0.visibility_flags)
    accept = ~(enough & (d0.see_through > F))
    assert np.array_equal(d.accept, accept) and 0 < (~accept).sum() < n
    assert accept[~enough & (d0.see_through > F)].all(), 'a box seen through on too few rays is kept'
    nms = cap.nms[0]
    assert sorted(nms['members'].tolist()) == np.nonzero(accept)[0].tolist(), 'a rejected detection is listed in no group'
    assert np.array_equal(d.keep, nms['keep'][:n].astype(bool) & accept)
    assert lines[0] == 'consistency: kept %d of %d (see_through > %g: %d)' % (accept.sum(), n, F, (~accept).sum()), lines
    assert lines[1].startswith('floor: ')
    known = d0.see_through[(d0.visibility_flags & VS.UNMEASURED) == 0]
    assert lines[2] == 'visibility: 4 scenes, median see_through %.2f, rejected %d' % (np.median(known), (~accept).sum()), lines
    assert lines[3].startswith('nms (3d IoU > 0.05, ranked by prob): kept %d of %d detections' % (d.keep.sum(), accept.sum())) and len(lines) == 4
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        DT.write_consistency_json(os.path.join(tmp, 'rows.json'), meta, DT.Detector(flags(), rt=rt, visibility=True, consistency=True).decode_all(parts)[1])
        rows = json.load(open(os.path.join(tmp, 'rows.json')))
    assert len(rows) == n and list(rows[0])[-4:] == ['see_through', 'occluded', 'support', 'visibility_flags'] and rows[0]['see_through'] == d0.see_through[0]


# ---- what the measure says of clean label boxes ------------------------------------------------------------------------------------------------
def label_boxes(seed, W=182, H=132):
    """Two noise-free scenes cast by the specification of the ray caster, their range maps by the specification, and the label boxes as
    detections -> (label [n, 7], corners [n, 8, 3], scene index, calib, dims, goff, range)."""
    from transferable3d_amd.consistency import calib_row
    ss = SS.generate(Runtime(device='cpu', lib=FF.FakeSceneLib()), range(1, 3), seed, width=W, height=H, noise_a=0.0, p_drop=0.0)
    cal = np.stack([calib_row(s['Rtilt'], s['K'], (W, H)) for s in ss.scenes])
    dims, goff = FV.grids([(W, H)] * 2, 4)
    points = np.concatenate([s['depth'] for s in ss.scenes])
    offsets = np.concatenate([[0], np.cumsum([len(s['depth']) for s in ss.scenes])])
    rng, _ = FV.scene_range_batch(points, offsets, cal, [0, 1], dims, goff, int(goff[-1]), 4)
    lab, kor, idx = [], [], []
    for s, sc in enumerate(ss.scenes):
        for l in sc['labels']:
            k, ob = SD.compute_box_3d(l['object']), l['object']
            lab.append([2 * ob.h, 2 * ob.w, 2 * ob.l, k[:, 0].mean(), k[:, 1].max(), k[:, 2].mean(), ob.heading_angle])
            kor.append(k)
            idx.append(s)
    return np.array(lab, np.float32), np.array(kor, np.float32), np.array(idx), cal, dims, goff, rng


def slid(lab, kor, d):
    """The boxes slid by the relative depth offset d, as mode 1 writes a moved row."""
    l2, k2 = lab.copy(), kor.copy()
    tx, tz = lab[:, 3].astype(np.float64), lab[:, 5].astype(np.float64)
    l2[:, 3], l2[:, 5] = (tx + d * tx).astype(np.float32), (tz + d * tz).astype(np.float32)
    k2[:, :, 0] = (kor[:, :, 0].astype(np.float64) + d * tx[:, None]).astype(np.float32)
    k2[:, :, 2] = (kor[:, :, 2].astype(np.float64) + d * tz[:, None]).astype(np.float32)
    return l2, k2


STEPS = (np.arange(9) - 4) * 0.025          # nine candidates up to a tenth of the distance either way


def test_a_box_pulled_towards_the_camera_is_seen_through_more_and_holds_less():
    """Seed 12, scenes 1 and 2 at 182 x 132, 11 label boxes.  Summed over the boxes, the specification counts through 66 and inside 990
    for the label boxes, through 225 and inside 933 for the boxes pulled two steps (5 % of their distance) towards the camera.

    The slide (mode 1, nine candidates, min_gain 4) is NOT offered by any command, and this is why: of the boxes displaced by two steps
    either way it brings back to within one step of the label 4 of 22 here, and at most 16 of 38 (seed 36) over the seeds 1 .. 46 tried
    -- never more than half.  Pulled towards the camera, a label box still holds the visible front of its object, so inside - through
    hardly falls (in 32 of these 46 seeds `inside` even rises); only a box pushed away loses its returns."""
    lab, kor, idx, cal, dims, goff, rng = label_boxes(12)
    run = lambda l, k, offsets, mode: FV.detect_visibility(l, k, idx, cal, dims, goff, rng, 4, offsets, 0.05, 0.1, 4, mode)
    here = run(lab, kor, [0.0], 0)[0][:, 0].sum(0)
    pulled = run(*slid(lab, kor, STEPS[2]), [0.0], 0)[0][:, 0].sum(0)
    print('label boxes %s, pulled %s' % (here.tolist(), pulled.tolist()))
    assert len(lab) == 11 and pulled[FV.THROUGH] > here[FV.THROUGH] and pulled[FV.INSIDE] < here[FV.INSIDE]
    assert (here[FV.THROUGH], here[FV.INSIDE], pulled[FV.THROUGH], pulled[FV.INSIDE]) == (66, 990, 225, 933)
    back = total = 0
    for d in (STEPS[2], STEPS[6]):
        out = run(*slid(lab, kor, d), STEPS, 1)
        applied = np.where((out[3] & abi.VIS_SNAPPED) != 0, STEPS[out[2]], 0.0)
        back += int((np.abs((1.0 + d) * (1.0 + applied) - 1.0) <= 0.025 * 1.0001).sum())
        total += len(lab)
    print('the slide brings back %d of %d' % (back, total))
    assert (back, total) == (4, 22), 'the finding the module docstring and the README state'
