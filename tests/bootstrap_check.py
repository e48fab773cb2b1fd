"""Shared cases of the bootstrap tests (t3d_bootstrap_weights, t3d_sunrgbd_eval_bootstrap, evaluate_sunrgbd --bootstrap): the CPU tests
run them through the specification library (fake_bootstrap.BootstrapSpec), the GPU tests through libt3d.so.  The reference of a replicate
is always fake_bootstrap's LITERAL expansion of the resampled data set, evaluated by the EXISTING entry point t3d_sunrgbd_eval through the
same runtime -- on the GPU the existing kernel on the expanded boxes, not the weighted curve under test."""
import os

import numpy as np

import fake_bootstrap as FB
import sunrgbd_eval_check as SC
from transferable3d_amd import bootstrap as BS, evaluate_sunrgbd as ES



def spec_rt():
    """A runtime on the specification library (every entry point the flows below reach)."""
    import fake_consistency as FK
    import fake_nms as FN
    import fake_sweep as FS
    from fake_detect import DetectDecodeSpec
    from fake_frustum import FakeFrustumLib
    from fake_sunrgbd_eval import FakeSunrgbdEvalLib
    from transferable3d_amd.engine import Runtime

    class SpecLib(FB.BootstrapSpec, FS.SweepSpec, FK.ConsistencySpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib, FakeSunrgbdEvalLib):
        pass
    return Runtime(device='cpu', lib=SpecLib())


N_IMG = 24                                   # images of a synthetic case; the last third holds no ground truth


def case(P, G, seed=0, n_img=N_IMG):
    """(det, gt) in the manner of sweep_check.eval_case, over more images: G boxes in the first two thirds of the images; P detections --
    jittered copies of the boxes (several per box) and clutter, some in images without ground truth; confidences on a grid of 1/20, so
    that they tie within and across images, with a NaN here and there."""
    r = np.random.RandomState(1000 * seed + 7 * P + G)
    par = lambda n: np.stack([r.uniform(-3, 3, n), r.uniform(1.5, 6, n), r.uniform(-1, 1, n), r.uniform(0.4, 2.0, n), r.uniform(0.4, 2.0, n),
                              r.uniform(0.4, 1.5, n), r.uniform(-np.pi, np.pi, n)], 1).reshape(n, 7)
    g_par, g_img = par(G), r.randint(0, 2 * n_img // 3, G)
    d_par, d_img = par(P), r.randint(0, n_img, P)
    if G and P:
        src = r.randint(0, G, P)
        copy = r.uniform(size=P) < 0.7
        jit = g_par[src] + np.concatenate([r.normal(size=(P, 3)) * [0.15, 0.15, 0.08], np.zeros((P, 3)), r.normal(size=(P, 1)) * 0.25], 1)
        d_par[copy], d_img[copy] = jit[copy], g_img[src][copy]
    conf = np.round(r.uniform(size=P) * 20.0) / 20.0
    conf[r.uniform(size=P) < 0.02] = np.nan
    return (SC.stack([SC.box(*p) for p in d_par], d_img, conf), SC.stack([SC.box(*p) for p in g_par], g_img))


def columns(det, gt, seed=0, n_img=N_IMG, stride=None):
    """(det_col, gt_col): image k sits in column perm[k] of a matrix of n_img + 3 columns (`stride` where given), except image 1, whose
    detections name a column beyond the matrix and whose boxes column -1: weight 0."""
    stride = n_img + 3 if stride is None else stride
    perm = np.random.RandomState(seed + 11).permutation(n_img).astype(np.int32)
    det_col, gt_col = perm[np.asarray(det['image'], np.int64)], perm[np.asarray(gt['image'], np.int64)]
    det_col[np.asarray(det['image']) == 1] = stride + 5
    gt_col[np.asarray(gt['image']) == 1] = -1
    return det_col, gt_col


def matrix(R, big, seed=0, n_img=N_IMG, stride=None):
    """int32 [R, stride]: hand-made rows first -- zeros on every third column, multiplicities 1 .. 3 elsewhere and `big` on one column;
    all ones; all zeros -- then rows drawn by the specification's hash; R == 1 is the first hand-made row alone.  The columns from
    n_img on hold a weight nobody may read."""
    stride = n_img + 3 if stride is None else stride
    r = np.random.RandomState(seed + 5)
    hand = r.randint(1, 4, n_img).astype(np.int32)
    hand[::3] = 0
    hand[int(r.choice(np.nonzero(hand)[0]))] = big
    rows = [hand, np.ones(n_img, np.int32), np.zeros(n_img, np.int32)][:R]
    if R > 3:
        rows += list(FB.weights(seed + 1, R - 3, n_img))
    w = np.full((R, stride), 9, np.int32)
    w[:, :n_img] = np.stack(rows)
    return w


def run(rt, det, gt, w, det_col, gt_col, threshold=0.25):
    """t3d_sunrgbd_eval_bootstrap through evaluate_sunrgbd._eval_prepare -> the evaluation's arrays plus 'boot'."""
    launch, fetch = ES._eval_prepare(det, gt, None, threshold, rt, boot=(BS.Weights.of(rt, w), det_col, gt_col))
    launch()
    return fetch()


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a if k != 'boot') and all(a['boot'][k].tobytes() == b['boot'][k].tobytes() for k in a['boot'])


def check_curves(rt, P, G, R, seed=0, exact=False):
    """One case against the literal expansion: integer outputs equal, ap within 1e-12 (exact: equal), the row of zeros 0 (the row of
    ones: check_ones, on columns that all lie inside the matrix), every output of the evaluation the bytes of a plain call, two calls equal bytes."""
    det, gt = case(P, G, seed)
    det_col, gt_col = columns(det, gt, seed)
    w = matrix(R, 1000 if P <= 65 else 7, seed)
    got = run(rt, det, gt, w, det_col, gt_col)
    assert same_bytes(got, run(rt, det, gt, w, det_col, gt_col)), 'two runs differ'
    plain = ES._eval_call(det, gt, None, 0.25, rt)
    for k, v in plain.items():
        assert got[k].tobytes() == v.tobytes(), k
    ref = FB.literal(lambda d, g: ES._eval_call(d, g, None, 0.25, rt), det, gt, det_col, gt_col, w)
    b = got['boot']
    for k in ('n_pos', 'n_tp', 'n_fp'):
        assert b[k].dtype == np.int64 and np.array_equal(b[k], ref[k]), (k, b[k], ref[k])
    err = np.abs(b['ap'] - ref['ap'])
    print('P %d G %d R %d: worst |ap - literal| %.3g, ap %s' % (P, G, R, err.max(), np.round(b['ap'][:4], 4)))
    assert (err <= (0.0 if exact else 1e-12)).all(), (b['ap'], ref['ap'])
    if R >= 3:
        assert b['ap'][2] == 0.0 and b['n_pos'][2] == 0 and b['n_tp'][2] == 0 and b['n_fp'][2] == 0
    if P == 0 or G == 0:
        assert (b['ap'] == 0.0).all()
    return got, ref


def check_ones(rt, P, G, seed=0):
    """A row of ones over columns that all lie inside the matrix: ap is the call's own ap, bit for bit, and the counts are the plain ones."""
    det, gt = case(P, G, seed)
    perm = np.random.RandomState(seed + 11).permutation(N_IMG).astype(np.int32)
    det_col, gt_col = perm[np.asarray(det['image'], np.int64)], perm[np.asarray(gt['image'], np.int64)]
    got = run(rt, det, gt, np.ones((2, N_IMG), np.int32), det_col, gt_col)
    b = got['boot']
    assert b['ap'][0].tobytes() == b['ap'][1].tobytes() == got['ap'][0].tobytes(), (b['ap'], got['ap'])
    assert list(b['n_pos']) == [G, G] and b['n_tp'][0] == got['is_tp'].sum() and b['n_fp'][0] == got['is_fp'].sum()


# ---- predictions on the golden scenes, in the label format of the result files --------------------------------------------------------
def golden_rows(root, idx_list, seed=0, jitter=0.12, drop=0.0):
    """{class: float64 [n, 9]} rows (image, h, w, l, tx, ty, tz, ry, score) made from the label boxes of the data set directory: every box
    twice, jittered (a duplicate), and one box of clutter per image and class; `drop`: the share of rows left out."""
    gt = ES.benchmark_groundtruth(str(root), idx_list)
    r = np.random.RandomState(seed)
    rows = {c: [] for c in ES.CLASS_NAMES['AB']}
    for g in range(len(gt['image'])):
        c = gt['classname'][g]
        if c not in rows:
            continue
        l, w, h = 2.0 * gt['coeffs'][g]
        cx, cy, cz = gt['centroid'][g]
        ry = float(np.arctan2(-gt['basis'][g][0, 1], gt['basis'][g][0, 0]))
        for _ in range(2):
            j = r.normal(size=3) * jitter
            rows[c].append([gt['image'][g], h, w, l, cx + j[0], h / 2.0 - cz + j[2], cy + j[1], ry + r.normal() * 0.1, r.uniform(0.3, 1.0)])
    for c in rows:
        for i in idx_list:
            rows[c].append([i, 1.0, 1.0, 1.0, r.uniform(-2, 2), 0.5, r.uniform(2, 5), 0.0, r.uniform(0.0, 0.6)])
        a = np.asarray(rows[c], np.float64).reshape(-1, 9)
        rows[c] = a[r.uniform(size=len(a)) >= drop]
    return rows


def held_of(rows):
    return {c: ES.boxes_from_label_format(a[:, 0].astype(np.int64), *[a[:, k] for k in range(1, 9)]) for c, a in rows.items()}


def write_pred_dir(path, rows):
    os.makedirs(path)
    for c, a in rows.items():
        with open(os.path.join(path, c + '_pred.txt'), 'w') as fh:
            for v in a:
                fh.write('%d %s -1 -1 -10 0 0 1 1 %s\n' % (int(v[0]), c, ' '.join(repr(float(x)) for x in v[1:])))
    return path
