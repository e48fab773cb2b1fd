"""CPU: the floor stage through the NumPy specification (tests/fake_floor.py): the estimator on cast scenes against the room it was
cast from, the options and their errors, the request, the stage's place among the stages behind the decode and its accept rule, and
the fields it adds to records and reports.  That the records of a run WITHOUT the flags are byte for byte what they were is shown by the
existing transcript tests, which this change leaves as they are; here a plain run is compared with a run that only measures, field by
field as bytes.  tests/floor_check.py's kernel checks run here through the specification too, so that the
checkers themselves are exercised without a device."""
import json

import numpy as np
import pytest

import detect_check as DC
import fake_consistency as FK
import fake_floor as FF
import fake_fuse as FU
import fake_nms as FN
import floor_check as FC
import scene_check as SK
import stages_check as SC
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from transferable3d_amd import abi, detect as DT, floor as FL, semisup_infer as SI, synth_scenes as SS, test_semisup as TS
from transferable3d_amd.engine import Runtime


class SpecLib(FF.FloorSpec, FK.ConsistencySpec, FU.DetectFuseSpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib, FF.FakeSceneLib):
    pass


@pytest.fixture(scope='module')
def rt():
    return Runtime(device='cpu', lib=SpecLib())


def flags():
    return TS.build_flags(DC.MODEL_FLAGS)


# ---- the estimator ---------------------------------------------------------------------------------------------------------------------
def test_the_specification_finds_the_floor_of_every_cast_scene():
    """Seed 1, ids 1..8, 182 x 132, cast by the NumPy specification of the ray caster with the generator's noise and drops: the plane at the
    inlier centroid lies within one bin (0.02 m: the histogram's resolution, by which the peak is located) of the room's floor, in all
    eight.  Measured: at most 6 mm; the smallest floor share 0.08 (id 8)."""
    ss = SS.generate(Runtime(device='cpu', lib=FF.FakeSceneLib()), range(1, 9), 1, width=182, height=132)
    assert len(ss.scenes) == 8
    o = FL.FloorOptions().kernel_options()
    assert o == FF.OPTIONS
    for sc in ss.scenes:
        plane, counts, hist = FF.scene_floor(sc['depth'], o)
        a, b, c, mx, my = plane[:5]
        z = a * mx + b * my + c
        print('scene %d: floor %.4f, room %.4f, share %.3f, slope %.4f, flags %d' % (sc['id'], z, sc['room'][4], counts[1] / counts[0], np.hypot(a, b), counts[3]))
        assert counts[3] in (0, abi.FLOOR_LEVEL) and abs(z - sc['room'][4]) <= 0.02, (sc['id'], z, sc['room'][4])
        assert hist.sum() <= counts[0] == len(sc['depth'])


def test_the_kernel_checks_hold_for_the_specification(rt):
    for S in (1, 3, 9):
        FC.check_batch(rt, S, 3 + 3 * (S % 2))
    FC.check_constructed(rt)
    FC.check_batch_independence(rt)
    FC.check_scene_floor_refusals(rt.lib)
    FC.check_detect_floor_refusals(rt.lib)
    for n in FC.DETECT_SIZES:
        for mode in (0, 1, 2):
            FC.check_detect_floor(rt, n, mode)


def test_the_library_refuses_what_the_specification_refuses():
    """No device needed: a refusal comes before any launch."""
    lib = abi.load()
    FC.check_scene_floor_refusals(lib)
    FC.check_detect_floor_refusals(lib)


def test_device_floor_wrapper_equals_the_specification(rt):
    import torch
    points, offsets = FC.batch((300, 0, 5000), 6, seed=5)
    plane, counts, host = FL.DeviceFloor(rt).estimate(torch.from_numpy(points), offsets)
    want = FF.scene_floor_batch(points, offsets)
    assert FC.same(plane.numpy(), want[0]) and FC.same(counts.numpy(), want[1]) and np.array_equal(host, want[1])
    assert counts[1, 3] == abi.FLOOR_NONE and counts[2, 3] == 0


# ---- options, flags, the request ---------------------------------------------------------------------------------------------------------
def test_options_are_checked():
    o = FL.FloorOptions()
    assert (o.bin, o.z_lo, o.z_hi, o.min_share, o.min_inliers, o.band, o.max_tilt, o.min_spread, o.min_det_ratio) == (0.02, -3.0, -0.2, 0.02, 50, 0.05, 5.0, 0.25, 0.05)
    assert o.n_bins == 140 and o.inv_bin == 1.0 / 0.02 and o.max_slope2 == np.tan(np.radians(5.0)) ** 2
    for kw in (dict(bin=0.0), dict(bin=-0.02), dict(bin=float('nan')), dict(range=(-1.0, -1.0)), dict(range=(-1.0, -2.0)), dict(range=(float('nan'), 0.0)),
               dict(min_share=1.5), dict(min_share=-0.1), dict(band=-0.01), dict(band=float('nan')), dict(max_tilt=-1.0), dict(max_tilt=90.0),
               dict(max_tilt=float('nan')), dict(bin=0.001), dict(min_inliers=-1), dict(min_spread=-1.0), dict(min_det_ratio=float('nan'))):
        with pytest.raises(ValueError):
            FL.FloorOptions(**kw)
    f = FL.check_options()
    assert not f.on and f.snap is None and f.snap_max == 0.3 and f.max_floor_gap is None
    assert FL.check_options(floor=True).on and FL.check_options(snap_floor='shift').on and FL.check_options(max_floor_gap=0.0).on
    f = FL.check_options(snap_floor='stretch', snap_floor_max=0.5, floor_bin=0.04, floor_range=(-2.0, -0.4), floor_max_tilt=3.0)
    assert (f.snap, f.snap_max, f.options.bin, f.options.n_bins, f.options.max_tilt) == ('stretch', 0.5, 0.04, 40, 3.0)
    for kw in (dict(snap_floor_max=0.2), dict(floor=True, snap_floor_max=0.2), dict(snap_floor='lift'), dict(snap_floor='shift', snap_floor_max=-0.1),
               dict(snap_floor='shift', snap_floor_max=float('nan')), dict(max_floor_gap=-0.01), dict(max_floor_gap=float('nan')), dict(floor_bin=0.02),
               dict(floor_range=(-3.0, -0.2)), dict(floor_min_share=0.1), dict(floor_band=0.05), dict(floor_max_tilt=5.0), dict(floor=True, floor_bin=-1.0)):
        with pytest.raises(ValueError):
            FL.check_options(**kw)
    for kw in (dict(snap_floor_max=0.2), dict(floor_band=0.1), dict(max_floor_gap=-1.0)):          # Detector checks them before it builds a model
        with pytest.raises(ValueError):
            DT.Detector(object(), **kw)
    assert set(FL.FLAGS) <= set(DT.STAGE_KEYWORDS) and DT.RECORD_GROUPS[-1] == DT.ROW_GROUPS[-1] == 'floor'


BASE = ['--idx_path', 'none', '--rgb_detection_path', 'none']


@pytest.mark.parametrize('argv,message', [
    (['--snap_floor_max', '0.2'], 'needs --snap_floor'), (['--floor_bin', '0.02'], 'needs --floor'), (['--floor_range', '-3', '-1'], 'needs --floor'),
    (['--floor_json', 'x.json'], 'needs --floor'), (['--max_floor_gap', '-0.5'], 'not negative'), (['--max_floor_gap', 'nan'], 'not negative'),
    (['--snap_floor', 'shift', '--snap_floor_max', '-1'], 'not negative'), (['--floor', '--floor_band', 'nan'], 'floor_band'),
    (['--floor', '--sweep'], 'does not go with --floor'), (['--sweep', '--snap_floor', 'stretch'], 'does not go with --snap_floor'),
    (['--sweep', '--max_floor_gap', '0.2'], 'does not go with --max_floor_gap'), (['--rescore_fit', 'm.json', '--floor'], 'does not go with --floor'),
    (['--rescore_fit', 'm.json', '--max_floor_gap', '0.1'], 'does not go with --max_floor_gap')])
def test_flag_errors_are_argument_errors(argv, message, capsys):
    with pytest.raises(SystemExit):
        DT.main(BASE + argv + DC.MODEL_FLAGS)
    assert message in capsys.readouterr().err


def test_autolabel_takes_the_flags(capsys):
    from transferable3d_amd import autolabel as AL
    base = ['--idx_path', 'none', '--classes', 'chair', '--out_dir', 'none']
    args, _ = AL.parse(base + ['--snap_floor', 'shift', '--max_floor_gap', '0.2', '--floor_json', 'f.json'] + DC.MODEL_FLAGS)
    assert args.snap_floor == 'shift' and args.max_floor_gap == 0.2 and args.floor_json == 'f.json' and not args.floor
    with pytest.raises(SystemExit):
        AL.parse(base + ['--floor_json', 'f.json'] + DC.MODEL_FLAGS)
    assert 'needs --floor' in capsys.readouterr().err
    records = [dict({'class': 'chair', 'detected': True, 'accepted': g <= 0.2}, floor_gap=g, floor_flags=0) for g in (0.1, -0.3, float('nan'), 0.25)]
    tests = SI.active_tests(FL.check_options(max_floor_gap=0.2))
    c = AL.count(records, ['chair'], tests)['chair']
    assert c['rejected_by'] == {'max_floor_gap': 2} and AL.rejected_by(tests, records)['max_floor_gap'].tolist() == [False, True, False, True]


def test_semisup_infer_and_evaluate_do_not_take_the_flags(capsys):
    from transferable3d_amd import evaluate_sunrgbd as ES
    with pytest.raises(SystemExit):
        SI.build_flags(['--device_decode', '--floor'] + DC.MODEL_FLAGS)
    with pytest.raises(SystemExit):
        ES.main(['--pred_dir', 'none', '--idx_path', 'none', '--floor'])
    assert 'unrecognized arguments: --floor' in capsys.readouterr().err


def test_request_is_checked():
    planes, counts = np.zeros((2, 8)), np.zeros((2, 4), np.int32)
    r = FL.FloorRequest(planes, counts, [0, 1, -1])
    assert len(r) == 3 and r.snap is None and r.snap_max == 0.3 and r.max_floor_gap is None and r.scene_index.dtype == np.int32
    for bad in (lambda: FL.FloorRequest(planes, counts, [0, 2]), lambda: FL.FloorRequest(planes, counts, [-2]),
                lambda: FL.FloorRequest(planes[:, :7], counts, [0]), lambda: FL.FloorRequest(planes, counts[:1], [0]),
                lambda: FL.FloorRequest(planes, counts, [0], snap='lift'), lambda: FL.FloorRequest(planes, counts, [0], snap_max=-1.0),
                lambda: FL.FloorRequest(planes, counts, [0], max_floor_gap=float('nan'))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="decode='device'"):
        SI.inference(None, None, None, None, 4, decode='host', floor=r)
    with pytest.raises(ValueError, match='floor request'):
        SI.DeviceStages(None, 4, 2, 16, floor=r)


# ---- the stage among the stages ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def world(rt):
    """Four generated scenes whose detector reports every labelled object twice, and a run that only measures."""
    ss = SK.scene_set(rt, 4, det_dup=1.0, det_miss=0.0, det_confuse=0.0, det_fp_per_image=0.0)
    scenes = [{'points': s['depth'], 'Rtilt': s['Rtilt'], 'K': s['K']} for s in ss.scenes]
    dets = [s['detections'] for s in ss.scenes]
    plain = DT.Detector(flags(), rt=rt).detect(scenes, dets, scene_ids=ss.ids)
    det = DT.Detector(flags(), rt=rt, floor=True)
    parts = [det.extract(scenes, dets, ss.ids)]
    meta, d = det.decode_all(parts)
    return dict(ss=ss, scenes=scenes, dets=dets, plain=plain, meta=meta, d=d, parts=parts, det=det)


def test_measuring_adds_fields_and_changes_nothing_else(rt, world):
    records = DT.Detector(flags(), rt=rt, floor=True).detect(world['scenes'], world['dets'], scene_ids=world['ss'].ids)
    n = 0
    for a, b in zip(world['plain'], records):
        assert len(a) == len(b)
        for r, q in zip(a, b):
            assert list(q)[:len(r)] == list(r) and list(q)[len(r):] == ['floor_gap', 'floor_flags']
            assert all(np.asarray(r[k]).tobytes() == np.asarray(q[k]).tobytes() for k in r)
            n += 1
    d, part = world['d'], world['parts'][0]
    assert n == len(d) >= 8 and d.unsnapped_label is None and d.accept is None and d.keep is None
    want = FF.detect_floor(d.label.astype(np.float32), d.corners.astype(np.float32), [m.scene for m in world['meta']],
                           part['floor']['plane'].numpy(), part['floor']['counts'].numpy(), 0, 0.3)
    assert FC.same(d.floor_gap, want[0]) and np.array_equal(d.floor_flags, want[1]) and np.isfinite(d.floor_gap).all()
    for s, sc in enumerate(world['ss'].scenes):
        p = part['floor']['plane'][s].numpy()
        assert abs(p[0] * p[3] + p[1] * p[4] + p[2] - sc['room'][4]) <= 0.02 and not part['floor']['counts_host'][s, 3] & abi.FLOOR_NONE
    rows = world['det'].floor_json_rows(world['parts'])
    json.dumps(rows)
    assert [r['scene'] for r in rows] == world['ss'].ids and all(r['floor'] and 0 < r['share'] <= 1 and r['rms'] < 0.02 and len(r['plane']) == 3 for r in rows)
    fields = DT.fields_of(d, 0, DT.RECORD_GROUPS, as_lists=True)
    assert list(fields) == ['floor_gap', 'floor_flags'] and fields['floor_gap'] == d.floor_gap[0]


def test_a_rejected_box_is_in_no_group_and_a_scene_without_a_floor_rejects_nothing(rt, world):
    d0, meta0 = world['d'], world['meta']
    n = len(d0)
    gaps = np.abs(d0.floor_gap)
    worst = int(np.argmax(gaps))
    lost = meta0[worst].scene                              # the scene that will have no floor: the one of the box furthest from its floor
    others = np.array([m.scene != lost for m in meta0])
    assert 2 <= others.sum() < n
    G = SC.between(gaps[others], int(others.sum()) // 2)
    lines = []
    det = DT.Detector(flags(), rt=rt, max_floor_gap=G, nms_iou=0.05, log=lines.append)
    parts = [det.extract(world['scenes'], world['dets'], world['ss'].ids)]
    parts[0]['floor']['counts'][lost, 3] = abi.FLOOR_NONE
    with SC.Stages(rt) as cap:
        meta, d = det.decode_all(parts)
    batches = (n + 3) // 4
    assert cap.entry_points == ['decode'] * batches + ['floor', 'nms'], cap.entry_points
    assert np.isnan(d.floor_gap[~others]).all() and (d.floor_flags[~others] == abi.DETECT_FLOOR_NO_FLOOR).all()
    assert FC.same(d.floor_gap[others], d0.floor_gap[others])
    accept = ~(others & (gaps > G))
    assert np.array_equal(d.accept, accept) and accept[~others].all() and 0 < (~accept).sum() < others.sum()
    assert gaps[worst] > G, 'the box furthest from a floor would be rejected, had its scene one'
    nms = cap.nms[0]
    assert sorted(nms['members'].tolist()) == np.nonzero(accept)[0].tolist(), 'a rejected detection is listed in no group'
    assert np.array_equal(d.keep, nms['keep'][:n].astype(bool) & accept)
    assert lines[0] == 'consistency: kept %d of %d (|floor_gap| > %g: %d)' % (accept.sum(), n, G, (~accept).sum()), lines
    known = d.floor_gap[others]
    assert lines[1] == 'floor: 3 of 4 scenes with a floor (level only: %d), median gap %+.2f m (abs %.2f), rejected %d (|gap| > %g)' % (
        int((parts[0]['floor']['counts_host'][:, 3] & abi.FLOOR_LEVEL != 0).sum()) - int(parts[0]['floor']['counts_host'][lost, 3] & abi.FLOOR_LEVEL != 0),
        np.median(known), np.median(np.abs(known)), (~accept).sum(), G), lines
    assert lines[2].startswith('nms (3d IoU > 0.05, ranked by prob): kept %d of %d detections' % (d.keep.sum(), accept.sum())) and len(lines) == 3


@pytest.mark.parametrize('snap', ['shift', 'stretch'])
def test_snapping_hands_the_next_stage_the_snapped_boxes(rt, world, snap):
    d0, n = world['d'], len(world['d'])
    lines = []
    det = DT.Detector(flags(), rt=rt, snap_floor=snap, snap_floor_max=0.25, nms_iou=0.05, nms_fuse=True, consistency=True, log=lines.append)
    parts = [det.extract(world['scenes'], world['dets'], world['ss'].ids)]
    with SC.Stages(rt) as cap:
        meta, d = det.decode_all(parts)
    batches = (n + 3) // 4
    assert cap.entry_points == ['decode', 'consistency'] * batches + ['floor', 'nms', 'fuse'], cap.entry_points
    part = parts[0]
    gap, flags_, lo, co = FF.detect_floor(d0.label.astype(np.float32), d0.corners.astype(np.float32), [m.scene for m in meta],
                                          part['floor']['plane'].numpy(), part['floor']['counts'].numpy(), FL.MODES[snap], 0.25)
    snapped = (flags_ & abi.DETECT_FLOOR_SNAPPED) != 0
    assert 0 < snapped.sum() < n and (flags_ & abi.DETECT_FLOOR_TOO_FAR).any(), flags_
    assert FC.same(d.floor_gap, d0.floor_gap) and np.array_equal(d.floor_flags, flags_)
    assert FC.same(d.unsnapped_label, d0.label) and FC.same(d.unsnapped_corners, d0.corners)
    f64 = lambda a: a.astype(np.float64)
    assert FC.same(d.raw_label, f64(lo)) and FC.same(d.raw_corners, f64(co)), 'the fusion read what the floor stage wrote'
    assert FC.same(cap.nms[0]['corners'][:n], co) and FC.same(cap.fuse[0]['label'][:n], lo)
    assert np.array_equal(d.raw_label[snapped, 4], f64((d0.floor_gap[snapped] + d0.label[snapped, 4]).astype(np.float32)))
    assert FC.same(d.reproj_iou, DT.Detector(flags(), rt=rt, consistency=True).decode_all(
        [det.extract(world['scenes'], world['dets'], world['ss'].ids)])[1].reproj_iou), 'consistency stays measured on the unsnapped box'
    assert lines[1].startswith('floor: 4 of 4 scenes with a floor') and lines[1].endswith(', snapped %d of %d boxes (%s, |gap| <= 0.25)' % (snapped.sum(), n, snap)), lines
    path = 'rows.json'
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        DT.write_consistency_json(os.path.join(tmp, path), meta, d)
        rows = json.load(open(os.path.join(tmp, path)))
    assert len(rows) == n and list(rows[0])[-2:] == ['floor_gap', 'floor_flags'] and rows[0]['floor_gap'] == d.floor_gap[0]
