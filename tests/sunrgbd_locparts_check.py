"""TEST INFRASTRUCTURE ONLY -- cases of the split of the localisation errors (t3d_sunrgbd_locparts, evaluate_sunrgbd.diagnose_class(parts=True),
--diagnose_parts) shared by tests/test_sunrgbd_locparts_cpu.py (the specification library) and tests/test_sunrgbd_locparts_gpu.py
(libt3d.so).  The expected values of the hand case are worked out on paper; the generated cases are sunrgbd_diagnose_check's, compared
with the specification library, whose results are computed once per process."""
import ctypes as C
import json
import math
import os

import numpy as np

import ref_sunrgbd_eval as R
import sunrgbd_diagnose_check as DK
import sunrgbd_eval_check as K
from fake_sunrgbd_locparts import FakeSunrgbdLocPartsLib
from transferable3d_amd import abi
from transferable3d_amd import evaluate_sunrgbd as ES
from transferable3d_amd.engine import Runtime

T_F, T_B = DK.T_F, DK.T_B
PART = {k: i for i, k in enumerate(abi.LOC_PARTS)}
DIAG_KEYS = DK.EVAL_KEYS + DK.DISCRETE + ('other_overlap', 'ap_fixed')
DISCRETE = ('part_counts', 'part_boxes')
LOC = abi.DIAG_KINDS.index('loc')
SPEC_BOUND = DK.SPEC_BOUND


def spec_rt():
    return Runtime(device='cpu', lib=FakeSunrgbdLocPartsLib())


def raw(rt, det, gt, other, t_f=T_F, t_b=T_B, parts=True):
    """One t3d_sunrgbd_locparts call -> host arrays of every output of the three structs (part_overlap [P,5], loc_error [P,6])."""
    r = ES._eval_call(det, gt, None, t_f, rt, other=other, bg_threshold=t_b, parts=parts)
    if parts:
        r['part_overlap'], r['loc_error'] = r['part_overlap'].reshape(-1, 5), r['loc_error'].reshape(-1, 6)
    return r


# ---- the hand case ------------------------------------------------------------------------------------------------------------------
# Six chairs in image 1, 10 m apart: unit cubes at x = 0, 10, 20, 30 and 4 x 1 x 1 boxes at x = 40, 50; every centre at (x, 5, 0).
# Nine detections, best first.  Two unit cubes shifted by s along one axis overlap by (1 - s) / (1 + s): 0.75 -> 1/7.
#   0  the cube at 0                         TP
#   1  the cube at 1/3                       DUP  (overlap 1/2 with the claimed box)
#   2  the cube at 10.75                     LOC 1/7: XY and CENTRE give 1; Z, SIZE and HEADING leave 1/7
#   3  the cube at 20.5, 0.5 up              LOC (1/2 . 1/2) / (2 - 1/4) = 1/7: XY alone and Z alone give (1/2) / (3/2) = 1/3, CENTRE 1
#   4  a 1 x 1 x 5 box at 30                 LOC 1/5: SIZE only
#   5  the 4 x 1 x 1 box at 40 turned 40 deg LOC 0.2414...: HEADING only (the pairing is straight: cos 40 > sin 40; same sizes)
#   6  the 4 x 1 x 1 box at 50 turned 80 deg LOC 0.1453...: the pairing swaps (cos 80 < sin 80): heading error 10 deg, size errors -log 4
#                                            and +log 4; HEADING gives a 1 x 4 on the 4 x 1 box, 1/7; SIZE gives the 1 x 4 box turned 80 deg,
#                                            that is 4 x 1 turned -10 deg, 0.7045...
#   7  the cube at -0.75                     LOC 1/7 on the CLAIMED box 0: repaired by XY and CENTRE, so removed there, never promoted
#   8  the cube at 9.25                      LOC 1/7 on box 1 behind detection 2: repaired by XY and CENTRE, removed there
# ap: tp fp fp ... over 6 boxes = 1/6.  ap_fixed[loc]: tp fp tp tp tp tp tp (7, 8 removed): 1/6 + 5/6 . 6/7.
#   XY, CENTRE  tp fp tp tp fp fp fp - -   precisions 1 1/2 2/3 3/4 3/5 3/6 3/7: 1/6 (1 + 3/4 + 3/4) = 5/12     repaired 4, boxes 2
#   Z           tp fp fp tp fp fp fp fp fp the second tp at 2/4: 1/6 (1 + 1/2) = 1/4                              repaired 1, boxes 1
#   SIZE        tp fp fp fp tp fp tp fp fp tps at 2/5 and 3/7, envelope 3/7 for both: 1/6 (1 + 6/7) = 13/42       repaired 2, boxes 2
#   HEADING     tp fp fp fp fp tp fp fp fp the second tp at 2/6: 1/6 (1 + 1/3) = 2/9                              repaired 1, boxes 1
LONG = (4.0, 1.0, 1.0)
HAND_GT = [(0.0, (1.0, 1.0, 1.0)), (10.0, (1.0, 1.0, 1.0)), (20.0, (1.0, 1.0, 1.0)), (30.0, (1.0, 1.0, 1.0)), (40.0, LONG), (50.0, LONG)]
#            x      z    l w h            ry (deg)  confidence
HAND_DET = [(0.0, 0.0, (1.0, 1.0, 1.0), 0.0, 0.95), (1.0 / 3.0, 0.0, (1.0, 1.0, 1.0), 0.0, 0.9), (10.75, 0.0, (1.0, 1.0, 1.0), 0.0, 0.85),
            (20.5, 0.5, (1.0, 1.0, 1.0), 0.0, 0.8), (30.0, 0.0, (1.0, 1.0, 5.0), 0.0, 0.75), (40.0, 0.0, LONG, 40.0, 0.7), (50.0, 0.0, LONG, 80.0, 0.65),
            (-0.75, 0.0, (1.0, 1.0, 1.0), 0.0, 0.6), (9.25, 0.0, (1.0, 1.0, 1.0), 0.0, 0.5)]
HAND_KINDS = [0, 4, 2, 2, 2, 2, 2, 2, 2]
OV40, OV80, OV80_SIZE = 0.241411724926506, 0.145381336190656, 0.704514252065184
S = 1.0 / 7.0
#                     xy   z    centre size       heading
HAND_PART_OVERLAP = [[1.0, 1.0, 1.0, 1.0, 1.0], [1.0, 0.5, 1.0, 0.5, 0.5], [1.0, S, 1.0, S, S], [1.0 / 3.0, 1.0 / 3.0, 1.0, S, S],
                     [0.2, 0.2, 0.2, 1.0, 0.2], [OV40, OV40, OV40, OV40, 1.0], [OV80, OV80, OV80, OV80_SIZE, S], [1.0, S, 1.0, S, S], [1.0, S, 1.0, S, S]]
L4, L5 = math.log(4.0), math.log(5.0)
HAND_LOC_ERROR = [[0, 0, 0, 0, 0, 0], [1.0 / 3.0, 0, 0, 0, 0, 0], [0.75, 0, 0, 0, 0, 0], [0.5, 0.5, 0, 0, 0, 0], [0, 0, 0, 0, L5, 0],
                  [0, 0, 0, 0, 0, math.radians(40.0)], [0, 0, -L4, L4, 0, math.radians(10.0)], [0.75, 0, 0, 0, 0, 0], [0.75, 0, 0, 0, 0, 0]]
HAND_AP, HAND_AP_LOC = 1.0 / 6.0, 1.0 / 6.0 + 5.0 / 7.0
HAND_AP_PART = {'xy': 5.0 / 12.0, 'z': 0.25, 'centre': 5.0 / 12.0, 'size': 13.0 / 42.0, 'heading': 2.0 / 9.0}
HAND_PART_COUNTS = {'xy': 4, 'z': 1, 'centre': 4, 'size': 2, 'heading': 1}
HAND_PART_BOXES = {'xy': 2, 'z': 1, 'centre': 2, 'size': 2, 'heading': 1}
# medians over the seven LOC detections: xy (0 0 0 .5 .75 .75 .75), every other column has at least four zeros
HAND_LINES = ['Localisation for CHAIR: loc n 7 | xy 0.50 z +0.00 | l +0% w +0% h +0% | heading 0.0 deg',
              'dAP(loc) for CHAIR: xy 25.00 z 8.33 centre 25.00 size 14.29 heading 5.56 | of loc 71.43 | repaired 4 1 4 2 1 of 7']


def hand_case(rows=None):
    rows = range(len(HAND_DET)) if rows is None else rows
    det = K.stack([K.box(HAND_DET[i][0], 5.0, HAND_DET[i][1], *HAND_DET[i][2], ry=math.radians(HAND_DET[i][3])) for i in rows], [1] * len(rows),
                  [HAND_DET[i][4] for i in rows])
    gt_all = K.stack([K.box(x, 5.0, 0.0, *size) for x, size in HAND_GT], [1] * len(HAND_GT))
    gt_all['classname'] = ['chair'] * len(HAND_GT)
    return det, gt_all


def check_hand_case(rt):
    det, gt_all = hand_case()
    r = ES.diagnose_class('chair', det, gt_all, T_F, T_B, rt=rt, classes=['chair', 'table'], parts=True)
    assert list(r['kind']) == HAND_KINDS and list(r['gtState']) == [1, 2, 2, 2, 2, 2]
    assert abs(r['apScore'] - HAND_AP) < 1e-15 and abs(r['apFixed']['loc'] - HAND_AP_LOC) < 1e-14
    assert r['partOverlap'].shape == (9, 5) and r['locError'].shape == (9, 6)
    assert np.abs(r['partOverlap'] - np.array(HAND_PART_OVERLAP)).max() < 1e-12, r['partOverlap']
    assert np.abs(r['locError'] - np.array(HAND_LOC_ERROR, np.float64)).max() < 1e-12, r['locError']
    assert list(r['apPart']) == list(abi.LOC_PARTS) == list(r['partCounts']) == list(r['partBoxes']) == list(r['dAPPart'])
    assert r['partCounts'] == HAND_PART_COUNTS and r['partBoxes'] == HAND_PART_BOXES
    for k, v in HAND_AP_PART.items():
        assert abs(r['apPart'][k] - v) < 1e-14 and abs(r['dAPPart'][k] - (v - HAND_AP)) < 1e-14, (k, r['apPart'][k], v)
    s = r['locSummary']
    assert s['tp']['n'] == 1 and s['loc']['n'] == 7 and s['loc']['xy'] == 0.5 and all(s['tp'][k] == 0.0 for k in abi.LOC_ERRORS)
    assert all(s['loc'][k] == 0.0 for k in abi.LOC_ERRORS[1:])
    # without parts the dictionary is what it was, and what both calls share is the same
    r0 = ES.diagnose_class('chair', det, gt_all, T_F, T_B, rt=rt, classes=['chair', 'table'])
    assert not set(r0) & {'partOverlap', 'locError', 'partCounts', 'partBoxes', 'apPart', 'dAPPart', 'locSummary'}
    for k, v in r0.items():
        assert np.array_equal(np.asarray(v), np.asarray(r[k]), equal_nan=True) if not isinstance(v, dict) else v == r[k], k


def write_hand_data_set(root):
    """The hand case as a data-set directory and prediction files -> (pred_dir, dataset_dir, idx_path)."""
    lab = os.path.join(str(root), 'data', 'training', 'label_dimension')
    pred = os.path.join(str(root), 'pred')
    os.makedirs(lab)
    os.makedirs(pred)
    with open(os.path.join(lab, '%06d.txt' % 1), 'w') as fh:
        fh.write(''.join(K.label_line('chair', (x, 5.0, 0.0), l / 2.0, w / 2.0, h / 2.0) + '\n' for x, (l, w, h) in HAND_GT))
    idx = os.path.join(str(root), 'data', 'training', 'val_data_idx.txt')
    with open(idx, 'w') as fh:
        fh.write('1\n')
    for name in ES.CLASS_NAMES['AB']:
        with open(os.path.join(pred, name + '_pred.txt'), 'w') as fh:
            if name == 'chair':
                fh.write(''.join(K.pred_line(1, 'chair', (x, 5.0, z), l / 2.0, w / 2.0, h / 2.0, s, ry=math.radians(ry)) + '\n'
                                 for x, z, (l, w, h), ry, s in HAND_DET))
    return pred, os.path.join(str(root), 'data'), idx


def check_hand_lines(rt, root):
    """The two logged lines, the JSON and the .npz of the hand case through `main` (the prediction files hold six decimals: the
    overlaps of the turned boxes move by 1e-6, far from every threshold)."""
    pred, data, idx = write_hand_data_set(root)
    lines = []
    out = os.path.join(str(root), 'diag.json')
    ES.main(['--pred_dir', pred, '--dataset_dir', data, '--idx_path', idx, '--test_on', 'AB', '--diagnose', '--diagnose_parts', '--diagnose_json', out,
             '--save_curves', os.path.join(str(root), 'curves')], rt=rt, log=lines.append)
    k = lines.index('AP Score for CHAIR: [16.6667]')
    assert lines[k + 1].startswith('Diagnosis for CHAIR: tp 1 cls 0 loc 7 both 0 dup 1 bkg 0 |') and lines[k + 2].startswith('dAP for CHAIR: ')
    assert lines[k + 3:k + 5] == HAND_LINES
    # a class without detections: nothing to take a median of
    k = lines.index('AP Score for TABLE: [0]')
    assert lines[k + 3:k + 5] == ['Localisation for TABLE: loc n 0 | xy - z - | l - w - h - | heading - deg',
                                  'dAP(loc) for TABLE: xy 0.00 z 0.00 centre 0.00 size 0.00 heading 0.00 | of loc 0.00 | repaired 0 0 0 0 0 of 0']
    # means over the ten classes: only the chair contributes
    assert lines[-2].startswith('Mean dAP: ') and lines[-1] == 'Mean dAP(loc): xy 2.50 z 0.83 centre 2.50 size 1.43 heading 0.56'
    assert len(lines) == 10 * 6 + 3
    s = json.load(open(out))
    assert s['loc_parts'] == list(abi.LOC_PARTS) and sorted(s['classes']) == sorted(ES.CLASS_NAMES['AB'])
    c = s['classes']['chair']
    assert c['parts']['partCounts'] == HAND_PART_COUNTS and c['parts']['partBoxes'] == HAND_PART_BOXES and list(c['parts']) == ['apPart', 'dAPPart', 'partCounts', 'partBoxes']
    for key, v in HAND_AP_PART.items():
        assert abs(c['parts']['apPart'][key] - v) < 1e-12 and abs(c['parts']['dAPPart'][key] - (v - HAND_AP)) < 1e-12
        assert abs(s['mean_dAP_parts'][key] - (v - HAND_AP) / 10.0) < 1e-12
    assert c['locSummary']['loc']['n'] == 7 and c['locSummary']['tp']['n'] == 1 and abs(c['locSummary']['loc']['xy'] - 0.5) < 1e-12
    assert s['classes']['table']['locSummary']['loc']['n'] == 0 and math.isnan(s['classes']['table']['locSummary']['loc']['xy'])
    z = np.load(os.path.join(str(root), 'curves', 'chair_pr.npz'))
    assert z['partOverlap'].shape == (9, 5) and z['locError'].shape == (9, 6) and list(z['kind']) == HAND_KINDS
    assert np.abs(z['partOverlap'] - np.array(HAND_PART_OVERLAP)).max() < 1e-5 and np.abs(z['locError'] - np.array(HAND_LOC_ERROR)).max() < 1e-5


# ---- the generated cases ------------------------------------------------------------------------------------------------------------
_CACHE = {}
MARGIN, TIE = 1e-6, 1e-9


def _offenders(spec, gaps):
    """The detections with a part overlap within MARGIN of t_f, or whose pairing is within TIE of a tie."""
    return np.nonzero((np.abs(spec['part_overlap'] - T_F) <= MARGIN).any(1) | (gaps <= TIE))[0]


def generated(which):
    """sunrgbd_diagnose_check.generated(which) -- its detections, boxes and decisions off their boundaries -- with, in addition, every
    detection that has a part overlap within 1e-6 of t_f or a pairing within 1e-9 of a tie moved to a clutter image id, on a copy: the
    cached case of the diagnosis' tests stays as it is.  -> {class: (det, gt, other, the specification's arrays, |p - q| per detection,
    the number moved)}, computed once."""
    if which not in _CACHE:
        rt, out = spec_rt(), {}
        n_images = (DK.SMALL if which == 'small' else DK.LARGE)['n_images']
        for c, (det, gt, other) in ((c, v[:3]) for c, v in DK.generated(which).items()):
            det = dict(det, image=np.array(det['image']))
            spec = raw(rt, det, gt, other)
            bad = _offenders(spec, rt.lib.last_pairing_gap)
            if len(bad):
                det['image'][bad] = n_images + 100000 + np.arange(len(bad))
                spec = raw(rt, det, gt, other)
            out[c] = (det, gt, other, spec, rt.lib.last_pairing_gap, len(bad))
        _CACHE[which] = out
    return _CACHE[which]


def check_conditions(which):
    """What the generated case must satisfy on the specification's own values before anything is compared with them."""
    cases = generated(which)
    repaired = np.zeros(5, np.int64)
    boxes_differ, moved = False, 0
    for c, (det, gt, other, spec, gaps, n_moved) in cases.items():
        assert len(_offenders(spec, gaps)) == 0, (which, c)
        repaired += spec['part_counts']
        boxes_differ |= len(set(spec['part_boxes'].tolist())) > 1
        moved += n_moved
    print('%s: %d detections moved to clutter images; repaired per part %s' % (which, moved, repaired.tolist()))
    if which == 'small':
        assert len(cases) == DK.N_CLASSES and repaired.min() >= 20, repaired
        assert boxes_differ
        P = [len(v[0]['confidence']) for v in cases.values()]
        assert min(P) > 256 and any(5 * p % 256 for p in P)                   # more than one block of the match kernel, a ragged last one
    else:
        P = len(cases[DK.LARGE_CLASS][0]['confidence'])
        assert P > 2048 and P % 1024 != 0                                   # ragged chunks of more than one element in the curve workgroups
    return repaired


def check_against_spec(rt, which, bound):
    """-> the worst |difference| of part_overlap, loc_error and ap_part."""
    worst = np.zeros(3)
    for c, (det, gt, other, spec, _, _) in generated(which).items():
        got = raw(rt, det, gt, other)
        for k in DK.DISCRETE + DISCRETE:
            assert np.array_equal(got[k], spec[k]), (which, c, k)
        assert np.array_equal(np.isnan(got['loc_error']), np.isnan(spec['loc_error'])), (which, c)
        with np.errstate(invalid='ignore'):
            d_err = np.abs(got['loc_error'] - spec['loc_error'])
        d_err = float(np.nanmax(np.where(got['loc_error'] == spec['loc_error'], 0.0, d_err), initial=0.0))     # (equal infinities differ by 0)
        d = np.array([float(np.abs(got['part_overlap'] - spec['part_overlap']).max(initial=0.0)), d_err, float(np.abs(got['ap_part'] - spec['ap_part']).max())])
        print('%s class %d: P %d G %d repaired %s boxes %s  worst |part_overlap diff| %.3e  |loc_error diff| %.3e  |ap_part diff| %.3e'
              % (which, c, len(det['confidence']), len(gt['image']), got['part_counts'].tolist(), got['part_boxes'].tolist(), d[0], d[1], d[2]))
        worst = np.maximum(worst, d)
        assert np.allclose(got['loc_error'], spec['loc_error'], rtol=0, atol=bound, equal_nan=True), (which, c, d_err, bound)
        assert (d <= bound).all(), (which, c, d, bound)
    print('generated %s: worst |part_overlap difference| %.3e, |loc_error difference| %.3e, |ap_part difference| %.3e, bound %.3e' % (which, *worst, bound))
    return tuple(worst)


def _angles_and_sizes(boxes, i):
    """(ry, l, w, h) of box i of a list made by sunrgbd_eval_check.box: basis rows (c, -s, 0), (s, c, 0), (0, 0, 1)."""
    b = boxes['basis'][i]
    return math.atan2(b[1][0], b[0][0]), 2.0 * boxes['coeffs'][i][0], 2.0 * boxes['coeffs'][i][1], 2.0 * boxes['coeffs'][i][2]


def second_route_overlaps(det, gt, gt_idx, rows):
    """part_overlap of the detections `rows` by another route than the specification's pairing code: the counterfactual boxes from
    heading angles and sizes (a turn of d between the headings pairs l with l iff |cos d| >= |sin d|), their overlaps with the matched
    boxes by ref_sunrgbd_eval.bb3d_overlap_close_form."""
    out = np.zeros((len(rows), 5))
    cf = [[] for _ in range(5)]
    for i in rows:
        g = int(gt_idx[i]) - 1
        ra, la, wa, ha = _angles_and_sizes(det, i)
        rb, lb, wb, hb = _angles_and_sizes(gt, g)
        (ax, ay, az), (bx, by, bz) = det['centroid'][i], gt['centroid'][g]
        straight = abs(math.cos(ra - rb)) >= abs(math.sin(ra - rb))
        cf[0].append(K.box(bx, by, az, la, wa, ha, ra))
        cf[1].append(K.box(ax, ay, bz, la, wa, ha, ra))
        cf[2].append(K.box(bx, by, bz, la, wa, ha, ra))
        cf[3].append(K.box(ax, ay, az, *((lb, wb) if straight else (wb, lb)), hb, ra))
        cf[4].append(K.box(ax, ay, az, *((la, wa) if straight else (wa, la)), ha, rb))
    boxes = ES.select_boxes({k: gt[k] for k in ('centroid', 'basis', 'coeffs')}, np.asarray([int(gt_idx[i]) - 1 for i in rows]))
    for f in range(5):
        out[:, f] = np.diag(R.bb3d_overlap_close_form(K.stack(cf[f]), boxes, only=np.eye(len(rows), dtype=bool)))
    return out


def _permuted(boxes, perm, negate):
    """The same boxes with their basis rows (and coeffs) permuted and one row negated."""
    out = dict(boxes)
    basis = np.array(boxes['basis'], np.float64)[:, perm, :]
    basis[:, negate, :] = -basis[:, negate, :]
    out['basis'], out['coeffs'] = basis, np.array(boxes['coeffs'], np.float64)[:, perm]
    return out


def check_properties(rt, bound, classes=(0, 7)):
    """On classes of the small generated case and on parts of the hand case, through `rt`."""
    cases = generated('small')
    for c in classes:
        det, gt, other = cases[c][:3]
        a = raw(rt, det, gt, other)
        # every output of the two existing structs is that of t3d_sunrgbd_diagnose on the same input, byte for byte
        e = raw(rt, det, gt, other, parts=False)
        for k in DIAG_KEYS:
            assert a[k].tobytes() == e[k].tobytes(), (c, k)
        # two runs give identical bytes
        b = raw(rt, det, gt, other)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (c, k)
        # a fix only removes false positives or adds true positives, and FIX_LOC dominates it rank by rank
        ap, loc = float(a['ap'][0]), float(a['ap_fixed'][DK.FIX['loc']])
        assert (a['ap_part'] >= ap - bound).all() and (a['ap_part'] <= loc + bound).all(), (c, ap, a['ap_part'], loc)
        is_loc = a['kind'] == LOC
        assert is_loc.sum() > 20
        assert np.array_equal(a['part_counts'], ((a['part_overlap'] >= T_F) & is_loc[:, None]).sum(0)), c
        assert (a['part_boxes'] <= a['part_counts']).all() and (a['part_boxes'] <= a['gt_counts'][1]).all()
        hit = a['gt_idx'] > 0
        assert not a['part_overlap'][~hit].any() and np.isnan(a['loc_error'][~hit]).all() and np.isfinite(a['loc_error'][hit]).all()
        assert (a['loc_error'][hit, 5] >= 0).all() and (a['loc_error'][hit, 5] <= math.pi / 4 + 1e-15).all() and (a['loc_error'][hit, 0] >= 0).all()
        # the overlaps by a second route.  The boxes are rebuilt from atan2 / cos / sin of the stored basis, a few ulp from it, and the
        # overlap moves by at most some ten times the change of a corner: 1e-12 leaves three orders of magnitude
        rows = np.nonzero(hit)[0][:60]
        want = second_route_overlaps(det, gt, a['gt_idx'], rows)
        assert np.abs(a['part_overlap'][rows] - want).max() <= max(bound, 1e-12), (c, np.abs(a['part_overlap'][rows] - want).max())
        # rows permuted with their coeffs and a row negated, on either side: the same boxes
        p = raw(rt, _permuted(det, [1, 2, 0], 0), gt, other)
        assert np.abs(p['part_overlap'] - a['part_overlap']).max() <= bound and np.allclose(p['loc_error'], a['loc_error'], rtol=0, atol=bound, equal_nan=True), c
        p = raw(rt, det, _permuted(gt, [1, 0, 2], 1), other)                 # the box's horizontal rows change places: so do its l and w errors
        assert np.abs(p['part_overlap'] - a['part_overlap']).max() <= bound
        assert np.allclose(p['loc_error'][:, [0, 1, 3, 2, 4, 5]], a['loc_error'], rtol=0, atol=bound, equal_nan=True), c
        for k in DK.DISCRETE + DISCRETE:
            assert np.array_equal(p[k], a[k]), (c, k)
    # every LOC detection a pure x-shift (0, 1, 2, 7, 8 of the hand case): XY and CENTRE repair them all, the other parts none
    det, gt_all = hand_case([0, 1, 2, 7, 8])
    gt = ES.select_boxes(gt_all, np.ones(len(HAND_GT), bool))
    gt.pop('classname')
    none = K.stack([])
    a = raw(rt, det, gt, none)
    assert list(a['kind']) == [0, 4, 2, 2, 2] and list(a['part_counts']) == [3, 0, 3, 0, 0] and list(a['part_boxes']) == [1, 0, 1, 0, 0]
    loc, ap = a['ap_fixed'][DK.FIX['loc']:DK.FIX['loc'] + 1].tobytes(), a['ap'].tobytes()
    assert loc != ap
    for f, want in enumerate([loc, ap, loc, ap, ap]):
        assert a['ap_part'][f:f + 1].tobytes() == want, f


def check_edge_cases(rt):
    det, gt_all = hand_case()
    gt = ES.select_boxes(gt_all, np.ones(len(HAND_GT), bool))
    gt.pop('classname')
    table = K.stack([K.box(70.0, 5.0, 0.0, 1.0, 1.0, 1.0)], [1])
    none_det, none = K.stack([], confidence=[]), K.stack([])
    zeros = lambda r: not r['part_counts'].any() and not r['part_boxes'].any() and not r['ap_part'].any()
    # P == 0
    r = raw(rt, none_det, gt, table)
    assert zeros(r) and r['part_overlap'].shape == (0, 5) and r['loc_error'].shape == (0, 6) and list(r['gt_counts']) == [0, 0, 6]
    # G == 0: no detection has a box
    r = raw(rt, det, none, table)
    assert zeros(r) and not r['part_overlap'].any() and np.isnan(r['loc_error']).all() and not r['gt_idx'].any()
    # Go == 0
    r = raw(rt, det, gt, none)
    assert list(r['part_counts']) == [4, 1, 4, 2, 1] and list(r['part_boxes']) == [2, 1, 2, 2, 1]
    assert np.abs(r['ap_part'] - [HAND_AP_PART[k] for k in abi.LOC_PARTS]).max() < 1e-14
    # nothing at all
    r = raw(rt, none_det, none, none)
    assert zeros(r) and r['ap'][0] == 0.0
    # a single detection of each kind: only a LOC detection can be repaired
    one = lambda b, conf=0.5: raw(rt, K.stack([b], [1], [conf]), gt, table)
    cube = lambda x, z=0.0: K.box(x, 5.0, z, 1.0, 1.0, 1.0)
    r = one(cube(0.0))                                                       # TP
    assert list(r['kind']) == [0] and zeros(dict(r, ap_part=r['ap_part'] - r['ap'][0])) and np.array_equal(r['part_overlap'], [[1.0] * 5])
    r = one(cube(10.75))                                                     # LOC
    assert list(r['kind']) == [2] and list(r['part_counts']) == [1, 0, 1, 0, 0] == list(r['part_boxes']) and r['ap'][0] == 0.0
    assert np.array_equal(r['ap_part'], [1.0 / 6.0, 0, 1.0 / 6.0, 0, 0]) and r['ap_part'][0] == r['ap_fixed'][DK.FIX['loc']]
    r = one(cube(70.0))                                                      # CLS: on the table, on no chair
    assert list(r['kind']) == [1] and zeros(r) and not r['part_overlap'].any() and np.isnan(r['loc_error']).all()
    r = one(cube(70.8))                                                      # BOTH (1/9 with the table)
    assert list(r['kind']) == [3] and zeros(r) and np.isnan(r['loc_error']).all()
    r = one(cube(85.0))                                                      # BKG
    assert list(r['kind']) == [5] and zeros(r) and np.isnan(r['loc_error']).all()
    r = one(cube(10.95))                                                     # BKG on its own box (1/39 < t_b): measured, never repaired
    assert list(r['kind']) == [5] and zeros(r) and np.array_equal(r['part_overlap'][0] >= T_F, [True, False, True, False, False])
    assert abs(r['loc_error'][0, 0] - 0.95) < 1e-12
    r = raw(rt, K.stack([cube(0.0), cube(1.0 / 3.0)], [1, 1], [0.9, 0.8]), gt, table)   # DUP
    assert list(r['kind']) == [0, 4] and zeros(dict(r, ap_part=r['ap_part'] - r['ap'][0])) and (r['part_overlap'][1] >= T_F).all()
    # a detection without volume (w = 0) at the place of box 1, a sliver (w = 1e-3) at box 3 and a sound LOC detection.  A box of volume 0
    # overlaps nothing, so the evaluation finds no box for it (gt_idx 0): its overlaps are 0 and its errors, the size errors among
    # them, are not finite; with t_b = 0 it is still a LOC detection, and the host's summary has to skip it
    gt_all2 = dict(gt, classname=['chair'] * len(HAND_GT))
    det3 = K.stack([K.box(10.0, 5.0, 0.0, 1.0, 0.0, 1.0), cube(20.5, 0.5), K.box(30.0, 5.0, 0.0, 1.0, 1e-3, 1.0)], [1, 1, 1], [0.9, 0.8, 0.7])
    d = ES.diagnose_class('chair', det3, gt_all2, T_F, 0.0, rt=rt, classes=['chair'], parts=True)
    assert list(d['kind']) == [2, 2, 2] and list(d['gtIdxAll'][np.argsort(d['sortIdx'])]) == [0, 3, 4] and d['locSummary']['loc']['n'] == 3
    assert not d['partOverlap'][0].any() and not np.isfinite(d['locError'][0]).any()
    assert abs(d['partOverlap'][2, PART['size']] - 1.0) < 1e-12 and abs(d['locError'][2, 3] - math.log(1e-3)) < 1e-12 and d['locError'][2, 2] == 0.0
    assert d['partCounts'] == {'xy': 1, 'z': 1, 'centre': 1, 'size': 1, 'heading': 0}
    # medians over the two detections that have a box: xy (0.5, 0), w (0, log 1e-3)
    assert d['locSummary']['loc']['xy'] == 0.25 and abs(d['locSummary']['loc']['w'] - 0.5 * math.log(1e-3)) < 1e-12
    s = ES.loc_summary(np.array([2, 2, 2], np.uint8), np.array([[0.1, 0, -np.inf, 0, 0, 0], [0.3, 0, 0.2, np.nan, 0, 0], [np.nan] * 6]))
    assert s['loc']['n'] == 3 and abs(s['loc']['xy'] - 0.2) < 1e-15 and s['loc']['l'] == 0.2 and s['loc']['w'] == 0.0 and s['tp']['n'] == 0 and math.isnan(s['tp']['xy'])


def host_structs(P=2, G=2, Go=2):
    """The three argument structs on host buffers of the right sizes (for the refusals, which come before anything is launched or read)."""
    a, d, keep = DK.host_structs(P, G, Go)

    def buf(dt, n, T):
        x = np.zeros(max(int(n), 1), dt)
        keep.append(x)
        return x.ctypes.data_as(C.POINTER(T))
    ws = abi.sunrgbd_locparts_workspace_bytes(P, G)
    q = abi.SunrgbdLocPartsArgs(0, C.cast(buf(np.uint8, ws, C.c_uint8), C.c_void_p), ws, buf(np.float64, 5 * P, C.c_double), buf(np.float64, 6 * P, C.c_double),
                                buf(np.int32, 5, C.c_int32), buf(np.int32, 5, C.c_int32), buf(np.float64, 5, C.c_double))
    return a, d, q, keep


def _longer(s):
    """A struct that says it is 16 bytes longer, with a byte in use behind the fields this side knows -> (pointer, what keeps it alive)."""
    n = C.sizeof(s)
    mem = (C.c_ubyte * (n + 16))()
    C.memmove(mem, C.byref(s), n)
    C.cast(mem, C.POINTER(C.c_uint32))[0] = n + 16
    mem[n + 4] = 1
    return C.cast(mem, C.POINTER(type(s))), mem


def check_refusals(lib):
    null = C.c_void_p(0)
    call = lambda a, d, q: lib.t3d_sunrgbd_locparts(a if not isinstance(a, C.Structure) else C.byref(a), d if not isinstance(d, C.Structure) else C.byref(d),
                                                    q if not isinstance(q, C.Structure) else C.byref(q), null)
    for k in range(3):                                                       # a short and a long struct, each of the three
        s = list(host_structs()[:3])
        s[k].struct_size -= 8
        assert call(*s) == abi.ERR_ABI, k
        s = list(host_structs()[:3])
        s[k], mem = _longer(s[k])
        assert call(*s) == abi.ERR_ABI, k
    for name in ('part_overlap', 'loc_error', 'part_counts', 'part_boxes', 'ap_part'):
        a, d, q, keep = host_structs()
        setattr(q, name, None)
        assert call(a, d, q) == -1, name                                     # a NULL output
    a, d, q, keep = host_structs()
    q.workspace_bytes -= 1
    assert call(a, d, q) == -1                                               # a small workspace
    a, d, q, keep = host_structs()
    q.workspace = None
    assert call(a, d, q) == -1
    a, d, q, keep = host_structs()
    q.reserved = 1
    assert call(a, d, q) == -1
    # whatever t3d_sunrgbd_diagnose refuses
    a, d, q, keep = host_structs()
    a.gt_difficult = keep[0].ctypes.data_as(abi.U8)
    assert call(a, d, q) == -1
    for t_b in (T_F, -0.01, float('nan')):
        a, d, q, keep = host_structs()
        d.bg_threshold = t_b
        assert call(a, d, q) == -1, t_b
    a, d, q, keep = host_structs()
    d.workspace_bytes -= 1
    assert call(a, d, q) == -1
    a, d, q, keep = host_structs()
    d.ap_fixed = None
    assert call(a, d, q) == -1
    a, d, q, keep = host_structs()
    d.Go = -1
    assert call(a, d, q) == -2
    a, d, q, keep = host_structs()
    a.workspace_bytes -= 1                                                   # ... and what t3d_sunrgbd_eval refuses
    assert call(a, d, q) == -1


# ---- command lines ------------------------------------------------------------------------------------------------------------------
NEW_LINES = ('Localisation for ', 'dAP(loc) for ', 'Mean dAP(loc): ')


def check_command_line(rt, root):
    """evaluate_sunrgbd --pred_dir on write_cli_data_set's tree: --diagnose_parts adds exactly the new lines behind the existing ones."""
    pred, data, idx, expected = K.write_cli_data_set(root)
    base = ['--pred_dir', pred, '--dataset_dir', data, '--idx_path', idx, '--test_on', 'B']
    plain, diag, lines = [], [], []
    ES.main(base, rt=rt, log=plain.append)
    assert plain == expected                                                 # without the flags: what it logs today
    out0, out1 = os.path.join(str(root), 'd0.json'), os.path.join(str(root), 'd1.json')
    ES.main(base + ['--diagnose', '--diagnose_json', out0], rt=rt, log=diag.append)
    ap, mean_ap = ES.main(base + ['--diagnose', '--diagnose_parts', '--diagnose_json', out1], rt=rt, log=lines.append)
    assert [l for l in lines if not l.startswith(NEW_LINES)] == diag and abs(mean_ap - 14.0 / 30.0) < 1e-12
    want = []
    for l in diag:
        want.append(l)
        if l.startswith('dAP for '):
            name = l.split()[2].rstrip(':')
            want += ['Localisation for %s: ' % name, 'dAP(loc) for %s: ' % name]
    want.append('Mean dAP(loc): ')
    assert len(lines) == len(want) and all(l.startswith(w) for l, w in zip(lines, want)), lines
    # no class of this tree has a localisation error
    assert 'Localisation for SOFA: loc n 0 | xy - z - | l - w - h - | heading - deg' in lines
    assert lines[-1] == 'Mean dAP(loc): xy 0.00 z 0.00 centre 0.00 size 0.00 heading 0.00'
    # the JSON without the flag is what it was; with it, it holds that and the new keys
    s0, s1 = json.load(open(out0)), json.load(open(out1))
    assert 'loc_parts' not in s0 and 'mean_dAP_parts' not in s0 and all('parts' not in c and 'locSummary' not in c for c in s0['classes'].values())
    assert {k: v for k, v in s1.items() if k not in ('loc_parts', 'mean_dAP_parts', 'classes')} == {k: v for k, v in s0.items() if k != 'classes'}
    for name, c in s1['classes'].items():
        assert {k: v for k, v in c.items() if k not in ('parts', 'locSummary')} == s0['classes'][name]


def check_parser_errors(rt, root):
    import pytest
    from transferable3d_amd import detect as DT
    pred, data, idx, _ = K.write_cli_data_set(root)
    base = ['--pred_dir', pred, '--dataset_dir', data, '--idx_path', idx]
    for extra in (['--diagnose_parts'], ['--official_eval', '--diagnose_parts'], ['--diagnose_parts', '--diagnose_bg', '0.05'],
                  ['--diagnose', '--diagnose_parts', '--bootstrap', '10']):
        with pytest.raises((SystemExit, ValueError)):
            ES.main(base + extra, rt=rt, log=lambda *a: None)
    needed = ['--idx_path', idx, '--rgb_detection_path', pred]
    for extra in (['--diagnose_parts'], ['--official_eval', '--diagnose_parts'], ['--diagnose', '--diagnose_parts']):
        with pytest.raises((SystemExit, ValueError)):
            DT.main(needed + extra, rt=rt, log=lambda *a: None)
    f = ES.parser().parse_args(['--idx_path', 'i'])
    assert f.diagnose_parts is False and ES.diagnose_options(ES.parser(), f) is None
    f = ES.parser().parse_args(['--idx_path', 'i', '--diagnose', '--diagnose_parts'])
    assert ES.diagnose_options(ES.parser(), f) == {'bg': 0.1, 'json': None, 'parts': True}
    f = ES.parser().parse_args(['--idx_path', 'i', '--diagnose'])
    assert ES.diagnose_options(ES.parser(), f)['parts'] is False
    f = DT.parser().parse_args(needed + ['--official_eval', '--diagnose', '--diagnose_parts'])
    assert f.diagnose and f.diagnose_parts


def check_detect_official_eval_diagnose_parts(rt, root):
    """detect --official_eval --diagnose --diagnose_parts end to end on the golden scenes: the lines of the run with --diagnose alone,
    plus the new ones."""
    import detect_check as DC
    from transferable3d_amd import detect as DT
    ids, folder, idx, dets = DC.write_data_set(root)
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--rgb_detection_path', folder, '--official_eval', '--diagnose'] + DC.MODEL_FLAGS
    diag, lines = [], []
    DT.main(base, rt=rt, log=diag.append)
    out = os.path.join(str(root), 'diag.json')
    DT.main(base + ['--diagnose_parts', '--diagnose_json', out], rt=rt, log=lines.append)
    assert [l for l in lines if not str(l).startswith(NEW_LINES)] == diag
    new = [l for l in lines if str(l).startswith(NEW_LINES)]
    assert len(new) == 2 * 10 + 1 and new[-1].startswith('Mean dAP(loc): ') and lines[-1] == new[-1]
    s = json.load(open(out))
    assert s['loc_parts'] == list(abi.LOC_PARTS) and set(s['mean_dAP_parts']) == set(abi.LOC_PARTS)
    for c in s['classes'].values():
        assert c['locSummary']['loc']['n'] == c['counts']['loc'] and c['locSummary']['tp']['n'] == c['counts']['tp']
        assert all(0 <= c['parts']['partBoxes'][k] <= c['parts']['partCounts'][k] <= c['counts']['loc'] for k in abi.LOC_PARTS)
    return new
