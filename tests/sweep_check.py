"""Shared cases of the threshold-sweep tests (t3d_detect_nms_sweep, t3d_sunrgbd_eval_sweep, detect --sweep): the CPU tests run them
through the specification library (fake_sweep.SweepSpec), the GPU tests through libt3d.so.  The reference of a configuration is always
the EXISTING entry point called on that configuration alone -- t3d_detect_nms on the restricted lists, t3d_sunrgbd_eval on the selected
detections -- through the same runtime, so on the GPU the references are the existing kernels and not the code under test."""
import os

import numpy as np
import torch

import fake_nms as FN
import fake_sweep as FS
import nms_check as NC
import sunrgbd_eval_check as SC
from transferable3d_amd import evaluate_sunrgbd as ES, nms as NMS

SIZES = (0, 1, 2, 63, 64, 65, 130)        # both sides of a wave and of a 64-bit mask word, more than two words, and an empty group
GRID_K = {1: [0.25], 4: [0.0, 0.25, 0.5, 1.0]}


# ---- the suppression ----------------------------------------------------------------------------------------------------------------
def nms_case(seed=51):
    """One call with a group of each of SIZES and three boxes in no group.  No margin rule: the references decide with the same fp32 IoU."""
    c = NC.Case('sweep_sizes', seed=seed)
    for size in SIZES:
        if size:
            c.add_group(size, dup=2 if size == 2 else 4, clutter=size // 8)
        else:
            c.groups.append([])
    c.add_unlisted(3)
    assert c.n % 64 != 0 and sorted(len(g) for g in c.groups) == sorted(SIZES)
    return c


def big_nms_case(seed=52):
    """One group of exactly T3D_DETECT_NMS_MAX_GROUP boxes (256 well-separated objects x 4 copies) beside a group of three."""
    c = NC.Case('sweep_1024', seed=seed)
    g = []
    for k in range(256):
        obj = NC.draw_object(c.r)
        obj[0], obj[2], obj[3:6] = 3.0 * (k % 16), 3.0 * (k // 16), c.r.uniform(0.4, 1.0, 3)
        g += [c.add_box(NC.draw_copy(c.r, obj), c.r.uniform(0, 1), obj) for _ in range(4)]
    c.groups.append(sorted(g))
    c.add_group(3)
    return c


def repaired_case(metric, thresholds, seed=53):
    """A small mixed case that keeps nms_check.MARGIN from EVERY threshold of the grid (for comparisons with the fp64 specification): the
    margin rule of nms_check is applied per threshold until a whole pass redraws nothing."""
    c = NC.Case('sweep_margins', seed=seed)
    for size in (0, 1, 2, 5, 9, 12, 7, 3):
        if size:
            c.add_group(size, dup=3, clutter=size // 5)
        else:
            c.groups.append([])
    c.add_unlisted(2)
    while True:
        before = c.redrawn
        for t in thresholds:
            if 0.0 < t < 1.0:
                c.repair(metric, t)
        if c.redrawn == before:
            break
    pairs = {}
    corners, score, _, _ = c.arrays()
    for g in c.groups:
        FN.group_pairs(corners.astype(np.float64), score, np.asarray(g, np.int64), pairs, NC.memo_iou)
    ious = [v[NC.METRIC_ID[metric]] for v in pairs.values() if v[0] == v[0]]
    assert all(abs(v - t) >= NC.MARGIN for v in ious for t in thresholds if 0.0 < t < 1.0)
    assert all(NC.MARGIN <= v <= 1.0 - NC.MARGIN or v == 0.0 for v in ious), 'a pair near the thresholds 0 or 1'
    return c


def configs(M, K, n, seed=0):
    """(config_threshold int32 [M], listed uint8 [M, n]): the threshold indices cycle through -1, 0 .. K-1; the rows are all ones, all
    zeros, then random with a growing share of ones."""
    r = np.random.RandomState(seed)
    ct = np.asarray([(m % (K + 1)) - 1 for m in range(M)], np.int32)
    if M == 1:
        ct[0] = 0
    listed = np.zeros((M, n), np.uint8)
    for m in range(M):
        listed[m] = 1 if m % 3 == 0 else 0 if m % 3 == 1 else (r.uniform(size=n) < 0.3 + 0.6 * (m / max(M - 1, 1)))
    return ct, listed


def up(rt, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)


def run_nms_sweep(rt, corners, score, offsets, members, thresholds, ct, listed, metric):
    """nms.DeviceNmsSweep on NumPy arrays -> (keep [M, n], n_kept [M]) as NumPy arrays."""
    dev = NMS.DeviceNmsSweep(rt)
    k = up(rt, corners.reshape(-1, 24)) if len(corners) else rt.zeros(0, 24)
    s = up(rt, score) if len(score) else rt.zeros(0)
    keep, n_kept = dev.run(k, s, offsets, members, thresholds, ct, None if listed is None else up(rt, listed), metric)
    return keep.cpu().numpy().copy(), n_kept.cpu().numpy().copy()


def reference_rows(rt, corners, score, offsets, members, thresholds, ct, listed, metric):
    """Per configuration, t3d_detect_nms (nms.DeviceNms) on the restricted lists into a zero-filled keep -> keep [M, n]."""
    n, M = len(score), len(ct)
    out = np.zeros((M, n), np.uint8)
    dev = NMS.DeviceNms(rt)
    k, s = up(rt, corners.reshape(-1, 24)), up(rt, score)
    for m in range(M):
        sel = np.ones(n, bool) if listed is None else listed[m] != 0
        go, mem = FS.restricted(offsets, members, sel)
        if ct[m] < 0:                                            # no suppression: every listed box of a group
            out[m, mem] = 1
            continue
        out[m] = dev.run(k, s, go, mem, thresholds[ct[m]], metric, fill=(0, -1, -1))[0].cpu().numpy()
    return out


def check_nms_sweep(rt, case, M, K, metric, with_listed=True, seed=0):
    corners, score, offsets, members = case.arrays()
    ct, listed = configs(M, K, case.n, seed)
    listed = listed if with_listed else None
    thresholds = GRID_K[K]
    keep, n_kept = run_nms_sweep(rt, corners, score, offsets, members, thresholds, ct, listed, metric)
    want = reference_rows(rt, corners, score, offsets, members, thresholds, ct, listed, metric)
    assert keep.shape == want.shape == (M, case.n)
    assert keep.tobytes() == want.tobytes(), [(m, np.nonzero(keep[m] != want[m])[0][:8]) for m in range(M) if not np.array_equal(keep[m], want[m])]
    assert np.array_equal(n_kept, want.sum(1)), (n_kept, want.sum(1))
    assert (keep[:, case.unlisted] == 0).all()
    return keep, n_kept, ct, listed


def moved_nms_sweep(rt, case, M, K, metric, seed=0):
    """The case's groups at other box indices of a larger call (interleaved with another case's boxes and groups, the group order
    reversed), the listed columns moved with them -> keep [M, case.n] mapped back."""
    other = nms_case(seed=77)
    k1, s1, _, _ = case.arrays()
    k2, s2, _, _ = other.arrays()
    total = case.n + other.n
    r = np.random.RandomState(seed + 5)
    perm = r.permutation(total)
    new1, new2 = np.sort(perm[:case.n]), np.sort(perm[case.n:])      # ascending, so that equal scores tie as before
    corners, score = np.zeros((total, 8, 3), np.float32), np.zeros(total, np.float32)
    corners[new1], score[new1], corners[new2], score[new2] = k1, s1, k2, s2
    groups = [sorted(int(new2[b]) for b in g) for g in other.groups] + [sorted(int(new1[b]) for b in g) for g in case.groups][::-1]
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    members = np.asarray([b for g in groups for b in g], np.int32)
    ct, listed1 = configs(M, K, case.n, seed)
    listed = (r.uniform(size=(M, total)) < 0.5).astype(np.uint8)
    listed[:, new1] = listed1
    keep, _ = run_nms_sweep(rt, corners, score, offsets, members, GRID_K[K], ct, listed, metric)
    return keep[:, new1]


# ---- the evaluation -----------------------------------------------------------------------------------------------------------------
def eval_case(P, G, seed=0):
    """(det, gt): G boxes over 8 images; P detections -- jittered copies of the boxes (several per box) and clutter, a sixth of them in
    images without ground truth; confidences on a grid of 1/20 (ties) with a NaN here and there."""
    r = np.random.RandomState(1000 * seed + 7 * P + G)
    par = lambda n: np.stack([r.uniform(-3, 3, n), r.uniform(1.5, 6, n), r.uniform(-1, 1, n), r.uniform(0.4, 2.0, n), r.uniform(0.4, 2.0, n),
                              r.uniform(0.4, 1.5, n), r.uniform(-np.pi, np.pi, n)], 1).reshape(n, 7)
    g_par, g_img = par(G), r.randint(0, 8, G)
    d_par, d_img = par(P), r.randint(0, 12, P)                       # images 8 .. 11 hold no ground truth
    if G and P:
        src = r.randint(0, G, P)
        copy = r.uniform(size=P) < 0.7
        jit = g_par[src] + np.concatenate([r.normal(size=(P, 3)) * [0.15, 0.15, 0.08], np.zeros((P, 3)), r.normal(size=(P, 1)) * 0.25], 1)
        d_par[copy], d_img[copy] = jit[copy], g_img[src][copy]
    conf = np.round(r.uniform(size=P) * 20.0) / 20.0
    conf[r.uniform(size=P) < 0.02] = np.nan
    return (SC.stack([SC.box(*p) for p in d_par], d_img, conf), SC.stack([SC.box(*p) for p in g_par], g_img))


def eval_masks(M, P, width=None, seed=0):
    """(masks uint8 [M, width], det_index or None): row 0 all ones, row 1 all zeros, the others random; with `width` > P the detections'
    columns are a random choice of the wider matrix's, in random order, and the other columns are noise."""
    r = np.random.RandomState(seed + 31 * M + P)
    rows = np.zeros((M, P), np.uint8)
    for m in range(M):
        rows[m] = 1 if m == 0 else 0 if m == 1 else (r.uniform(size=P) < r.uniform(0.1, 0.9))
    if width is None:
        return rows, None
    index = r.permutation(width)[:P].astype(np.int32)
    wide = (r.uniform(size=(M, width)) < 0.5).astype(np.uint8)
    wide[:, index] = rows
    return wide, index


def run_eval_sweep(rt, det, gt, masks, det_index, threshold=0.25):
    """t3d_sunrgbd_eval_sweep through evaluate_sunrgbd._eval_prepare -> its four arrays plus 'evaluation': what the evaluation wrote."""
    launch, fetch = ES._eval_prepare(det, gt, None, threshold, rt, sweep=(up(rt, masks), det_index))
    launch()
    return fetch(evaluation=True)


def check_eval_sweep(rt, P, G, M, wide=False, seed=0, exact=False):
    det, gt = eval_case(P, G, seed)
    masks, index = eval_masks(M, P, width=P + 37 if wide else None, seed=seed)
    got = run_eval_sweep(rt, det, gt, masks, index)
    again = run_eval_sweep(rt, det, gt, masks, index)
    assert all(got[k].tobytes() == again[k].tobytes() for k in ('ap', 'n_det', 'n_tp', 'n_fp')), 'two runs differ'
    plain = ES._eval_call(det, gt, None, 0.25, rt)
    for k, v in plain.items():                                       # every output of the evaluation: the bytes of a plain call
        assert got['evaluation'][k].tobytes() == v.tobytes(), k
    cols = np.arange(P) if index is None else index
    worst = 0.0
    for m in range(M):
        sel = np.nonzero(masks[m][cols] != 0)[0]
        ref = ES._eval_call(ES.select_boxes(det, sel), gt, None, 0.25, rt)
        assert (got['n_det'][m], got['n_tp'][m], got['n_fp'][m]) == (len(sel), int(ref['is_tp'].sum()), int(ref['is_fp'].sum())), (m, P, G)
        err = abs(got['ap'][m] - ref['ap'][0])
        worst = max(worst, err)
        assert err <= (0.0 if exact else 1e-12), (m, got['ap'][m], ref['ap'][0])
    assert got['ap'][0].tobytes() == plain['ap'][0].tobytes(), 'the row of ones is not the evaluation'
    if M > 1:
        assert got['ap'][1] == 0.0 and got['n_det'][1] == 0
    if P == 0 or G == 0:
        assert (got['ap'] == 0.0).all()
    return 'P %d G %d M %d%s: worst |ap - reference| %.3g, AP of all %.4f' % (P, G, M, ' wide' if wide else '', worst, got['ap'][0])


# ---- scene-level flow ---------------------------------------------------------------------------------------------------------------
# On the specification libraries the run's same-group 3-D IoUs are 0.289 0.540 0.631 0.646 0.689 0.695 0.771 0.849 0.890 and its reproj_iou values
# 0.206 .. 0.289 | 0.323 .. 0.471: the grid's values keep 0.01 from all of them, and each removes some detections and leaves some.
SWEEP_FLAGS = ['--sweep', '--sweep_nms_iou', 'off', '0.25', '0.66', '--sweep_min_reproj_iou', 'off', '0.3']


def check_flow(rt, root, exact):
    """detect --sweep on the duplicated golden scenes: every row's per-class AP and detection counts equal those of a separate detect run
    with that row's flags followed by evaluate_sunrgbd.evaluate; the baseline is the plain run's --official_eval; the log and the JSON
    say the same.  -> report lines."""
    import json
    import detect_check as DC
    from transferable3d_amd import detect as DT
    from transferable3d_amd.constants import class2type
    quiet = lambda *a: None
    ids, folder, idx, dets = NC.write_duplicated(root)
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS
    logged = []
    path = os.path.join(str(root), 'sweep.json')
    result = DT.main(base + SWEEP_FLAGS + ['--sweep_json', path, '--sweep_top', '3'], rt=rt, log=logged.append)
    assert logged[0].startswith('consistency: kept ')                 # the plain run's own line (the measures are on: a --sweep_min_* is given)
    logged = logged[1:]
    classes = ES.CLASS_NAMES['AB']
    assert len(result.rows) == 6 and result.rows[0] == (None, None, None, None) and result.rows[1] == (None, 0.3, None, None)
    assert result.rows[2] == (0.25, None, None, None) and result.rows[5] == (0.66, 0.3, None, None)
    report = []
    for m, row in enumerate(result.rows):
        flags = [] if result.table()[m]['flags'] == '(no flags)' else result.table()[m]['flags'].split()
        lines = []
        p = DT.main(base + flags, rt=rt, log=quiet)
        names = [class2type[int(c)] for c in p[10]]
        held = ES.official_predictions(sorted(set(classes) | set(names)), p, names)
        ap, mean = ES.evaluate(None, str(root), idx, 'AB', rt=rt, log=lines.append, predictions=held)
        for c in classes:
            err = abs(result.ap[c][m] - ap[c])
            assert err <= (0.0 if exact else 1e-12), (row, c, result.ap[c][m], ap[c])
            assert result.n_det[c][m] == len(held[c]['confidence']), (row, c)
            assert result.n_tp[c][m] + result.n_fp[c][m] == result.n_det[c][m]
        assert abs(result.mean_ap[m] - mean) <= 1e-12 and result.kept[m] == len(names), (row, result.kept[m], len(names))
        report.append('%s: mAP %.6f, %d detections' % (result.table()[m]['flags'], mean, len(names)))
        if m == 0:                                                   # the baseline states what --official_eval of the plain run prints
            plain = [l for l in lines if l.startswith('Mean AP Score')][0]
            shown = plain[plain.index('[') + 1:plain.index(']')]
            assert logged[1].startswith('baseline: mAP %s | ' % shown), (logged[1], plain)
    kept = [int(k) for k in result.kept]
    assert len(set(kept)) >= 3 and min(kept) > 0, kept                # the suppression and the filter both remove something, never all
    assert len(set(round(float(v), 9) for v in result.mean_ap)) >= 2, result.mean_ap
    assert logged[0] == 'sweep: 6 configurations over %d detections of 10 classes' % kept[0], logged[0]
    order = result.ranking()
    assert all((result.mean_ap[a], -a) >= (result.mean_ap[b], -b) for a, b in zip(order, order[1:]))
    assert len([l for l in logged if l[:4].strip().endswith('.')]) == 3 and logged[2].startswith('  1. %s: mAP ' % result.table()[order[0]]['flags'])
    assert logged[5] == 'best: ' + result.table()[order[0]]['flags'] and 'written to' in logged[6]
    js = json.load(open(path))
    assert len(js['rows']) == 6 and js['best']['index'] == order[0] and js['baseline']['kept'] == kept[0]
    assert [r['mean_ap'] for r in js['rows']] == [float(v) for v in result.mean_ap] and js['rows'][3]['options'] == {
        'nms_iou': 0.25, 'min_reproj_iou': 0.3, 'min_mask_in_box': None, 'min_seg_box_iou': None}
    return report + logged
