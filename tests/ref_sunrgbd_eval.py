"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 restatement of the official SUN-RGBD detection protocol, statement by statement after the
reference's MATLAB files (evaluation/sunrgbd/detection/*.m, sunrgbd/SUNRGBDtoolbox/mBB/*): boxes are dicts {'centroid', 'basis' (3x3,
rows), 'coeffs'}.  The footprint intersection is a Sutherland-Hodgman vertex list + shoelace sum, as cuboidIntersectionVolume.c does
with gpc's output -- NOT the boundary integral of csrc/sunrgbd_eval.hip.  MATLAB and Octave are not available, so nothing here is
recorded from the reference; it is a second, independent reading of the same files."""
import numpy as np

EPS = 2.0 ** -52


def get_corners_of_bb3d(centroid, basis, coeffs):
    """get_corners_of_bb3d.m:14-44 (flip_towards_viewer :46-53) -> corners [8,3]."""
    basis, coeffs, centroid = np.array(basis, np.float64), np.array(coeffs, np.float64), np.array(centroid, np.float64)
    inds = np.argsort(-np.abs(basis[:, 0]), kind='stable')                  # :17  sort(abs(basis(:,1)), 'descend')
    basis, coeffs = basis[inds], coeffs[inds]                               # :18-19
    inds = np.argsort(-np.abs(basis[1:3, 1]), kind='stable')                # :21
    if inds[0] == 1:                                                        # :22-25
        basis[1:3] = basis[1:3][::-1].copy()
        coeffs[1:3] = coeffs[1:3][::-1].copy()
    with np.errstate(invalid='ignore', divide='ignore'):
        points = centroid / np.sqrt(np.sum(centroid ** 2))                  # :47
    proj = np.array([points[0] * basis[r, 0] + points[1] * basis[r, 1] + points[2] * basis[r, 2] for r in range(3)])   # :49
    flip = proj > 0                                                         # :51
    basis[flip] = -basis[flip]                                              # :52
    coeffs = np.abs(coeffs)                                                 # :31
    sgn = [(-1, 1, 1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, -1), (1, 1, -1), (1, -1, -1), (-1, -1, -1)]      # :33-41
    corners = np.zeros((8, 3))
    for k, (a, b, c) in enumerate(sgn):
        corners[k] = (a * basis[0]) * coeffs[0] + (b * basis[1]) * coeffs[1] + (c * basis[2]) * coeffs[2]
    return corners + centroid                                               # :43


def to_vector(box):
    """bb3dOverlapCloseForm.m:17-30: x1 y1 x2 y2 x3 y3 x4 y4 zMin zMax."""
    k = get_corners_of_bb3d(box['centroid'], box['basis'], box['coeffs'])
    return np.concatenate([k[0:4, 0:2].reshape(-1), [min(k[0, 2], k[7, 2]), max(k[0, 2], k[7, 2])]])


def cuboid_volume(bb):
    """cuboidVolume.m:3-5 on one 10-vector."""
    dis = (bb[[0, 1, 4, 5]] - bb[[2, 3, 2, 3]]) ** 2
    return (bb[9] - bb[8]) * np.sqrt((dis[0] + dis[1]) * (dis[2] + dis[3]))


def _ccw(poly):
    a = 0.0
    for i in range(len(poly)):
        (x0, y0), (x1, y1) = poly[i], poly[(i + 1) % len(poly)]
        a += x0 * y1 - y0 * x1
    return poly if a >= 0 else poly[::-1]


def clip_convex(subject, clip):
    """Sutherland-Hodgman: the vertex list of subject ∩ clip (both convex, any orientation), standing in for gpc_polygon_clip (GPC_INT)."""
    out = _ccw([tuple(p) for p in subject])
    clip = _ccw([tuple(p) for p in clip])
    for i in range(len(clip)):
        (cx0, cy0), (cx1, cy1) = clip[i], clip[(i + 1) % len(clip)]
        ex, ey = cx1 - cx0, cy1 - cy0
        side = lambda p: ex * (p[1] - cy0) - ey * (p[0] - cx0)
        inp, out = out, []
        for j in range(len(inp)):
            a, b = inp[j], inp[(j + 1) % len(inp)]
            da, db = side(a), side(b)
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                t = da / (da - db)
                out.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
        if not out:
            break
    return out


def cuboid_intersection_volume(b1, b2):
    """cuboidIntersectionVolume.c:62-88 for one pair of 10-vectors."""
    z_overlap = min(b1[9], b2[9]) - max(b1[8], b2[8])                       # :64
    if not z_overlap > 0:                                                   # :66
        return 0.0
    v = clip_convex(b1[:8].reshape(4, 2), b2[:8].reshape(4, 2))             # :70
    m = len(v)
    if m <= 2:                                                              # :73
        return 0.0
    area = v[m - 1][0] * v[0][1] - v[m - 1][1] * v[0][0]                    # :83
    for k in range(1, m):                                                   # :84-87
        area += v[k - 1][0] * v[k][1] - v[k - 1][1] * v[k][0]
    return z_overlap * 0.5 * abs(area)                                      # :88


def overlap(v1, v2):
    """bb3dOverlapCloseForm.m:41-58 for one pair of 10-vectors.  Two boxes of volume 0: 0 (MATLAB: 0 / 0)."""
    inter = cuboid_intersection_volume(v1, v2)
    if inter == 0.0:
        return 0.0
    return inter / (cuboid_volume(v1) + cuboid_volume(v2) - inter)


def _box(boxes, i):
    return {k: np.asarray(boxes[k])[i] for k in ('centroid', 'basis', 'coeffs')}


def bb3d_overlap_close_form(bb1, bb2, only=None):
    """bb3dOverlapCloseForm.m -> dense [P,G].  `only` (bool [P,G]): the entries to compute, the others stay 0 -- computePRCurve3D.m:30-31
    zeroes every entry that is not on the same image before any is used, so the full-scale test does not clip 10^7 pairs in Python."""
    P, G = len(bb1['coeffs']), len(bb2['coeffs'])
    if P == 0 or G == 0:
        return np.zeros((P, G))
    v1 = [to_vector(_box(bb1, i)) for i in range(P)]
    v2 = [to_vector(_box(bb2, j)) for j in range(G)]
    m = np.zeros((P, G))
    pairs = np.argwhere(only) if only is not None else [(i, j) for i in range(P) for j in range(G)]
    for i, j in pairs:
        m[i, j] = overlap(v1[i], v2[j])
    return m


def get_average_precision(precision, recall):
    """get_average_precision.m:15-23."""
    mrec = np.concatenate([[0.0], recall, [1.0]])                           # :15
    mpre = np.concatenate([[0.0], precision, [0.0]])                        # :16
    for ii in range(len(mpre) - 2, -1, -1):                                 # :18-20  (MATLAB's max ignores a NaN)
        mpre[ii] = np.fmax(mpre[ii], mpre[ii + 1])
    ii = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1                           # :22
    return float(np.sum((mrec[ii] - mrec[ii - 1]) * mpre[ii]))              # :23


def compute_pr_curve_3d(det, gt, difficult=None, threshold=0.25, same_image_only=False):
    """computePRCurve3D.m for ground truth that is already of one class.  Everything is returned in the script's own order: isTp, isFp,
    gtAssignment in file order, the rest in sorted order; `allOverlaps` after the same-image mask.  P == 0 or G == 0: the values the
    entry point defines (every detection a false positive, recall 0 when G == 0, AP 0)."""
    conf = np.asarray(det['confidence'], np.float64)
    P, G = len(conf), len(gt['image'])
    is_difficult = np.zeros(G, bool) if difficult is None else np.asarray(difficult).astype(bool)       # :14
    sort_idx = np.argsort(-conf, kind='stable')                             # :20
    image_ids = np.asarray(det['image'])[sort_idx]                          # :23
    sorted_det = {k: np.asarray(det[k])[sort_idx] for k in ('centroid', 'basis', 'coeffs')}             # :22-23
    on_same_image = image_ids[:, None] == np.asarray(gt['image'])[None, :]  # :30
    all_overlaps = bb3d_overlap_close_form(sorted_det, gt, on_same_image if same_image_only else None)  # :28
    all_overlaps[~on_same_image] = 0                                        # :31
    if G > 0:
        gt_idx = np.argmax(all_overlaps, 1) + 1 if P else np.zeros(0, np.int64)                         # :32 (first index of the maximum)
        max_overlaps = all_overlaps[np.arange(P), gt_idx - 1] if P else np.zeros(0)
    else:
        gt_idx, max_overlaps = np.zeros(P, np.int64), np.zeros(P)
    gt_idx = gt_idx.copy()
    gt_idx[max_overlaps < EPS] = 0                                          # :33
    gt_idx_all = gt_idx.copy()                                              # :34
    is_overlapping = max_overlaps >= threshold                              # :35
    gt_idx[~is_overlapping] = 0                                             # :36
    unique_gt_idx, first_assignment = np.unique(gt_idx, return_index=True)  # :39  unique(gtIdx, 'first')
    is_first = np.zeros(P, bool)
    is_first[first_assignment] = True                                       # :40-41
    is_first &= gt_idx > 0                                                  # :42
    tmp_assign = np.zeros(P, np.int64)
    tmp_assign[first_assignment] = unique_gt_idx                            # :45-46
    gt_assignment = np.zeros(P, np.int64)
    gt_assignment[sort_idx] = tmp_assign                                    # :49
    is_missed = np.ones(G, bool)                                            # :62
    is_missed[unique_gt_idx[unique_gt_idx > 0] - 1] = False                 # :63
    tp = is_first & is_overlapping                                          # :67
    fp = ~tp                                                                # :68
    dc = (gt_idx != 0) & (is_difficult[np.maximum(1, gt_idx) - 1] if G else np.zeros(P, bool))          # :69
    tp[dc] = False                                                          # :70
    fp[dc] = False                                                          # :71
    is_tp, is_fp = np.zeros(P, bool), np.zeros(P, bool)
    is_tp[sort_idx], is_fp[sort_idx] = tp, fp                               # :72-75
    sum_fp, sum_tp = np.cumsum(fp.astype(np.float64)), np.cumsum(tp.astype(np.float64))                 # :78-79
    with np.errstate(invalid='ignore', divide='ignore'):
        recall = sum_tp / np.float64(np.sum(~is_difficult)) if G else np.zeros(P)                       # :80
        precision = sum_tp / (sum_fp + sum_tp)                              # :81
    return {'apScore': get_average_precision(precision, recall), 'precision': precision, 'recall': recall, 'isTp': is_tp, 'isFp': is_fp,
            'isMissed': is_missed, 'gtAssignment': gt_assignment, 'maxOverlaps': max_overlaps, 'gtIdxAll': gt_idx_all, 'sortIdx': sort_idx,
            'allOverlaps': all_overlaps}
