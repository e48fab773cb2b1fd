"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_detect_ensemble (include/t3d.h, csrc/ensemble.hip): `ensemble`
is the rule on arrays, DetectEnsembleSpec the entry point behind the ctypes struct on host pointers, so that ensemble.DeviceEnsemble,
semisup_infer.inference(decode='device', views=...) and transferable3d_amd/detect.py --tta run end to end through
Runtime(device='cpu', lib=FakeEnsembleLib())."""
import math

import numpy as np

import fake_fuse as FF
import fake_nms as FN
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

PI = math.pi
MAX_VIEWS = 8
wrap, align, usable = FF.wrap, FF.align, FF.usable


def unmirror(row, angle):
    """The fp32 view label of a mirrored view: `row` (h, w, l, tx, ty, tz, ry) fp32 mirrored back across the vertical plane that
    t3d_batch_assemble's flip used, in fp64, the three changed entries rounded to fp32 once."""
    h, w, l, tx, ty, tz, ry = (float(v) for v in row)
    a = float(angle)
    c, s = (math.cos(a), math.sin(a)) if math.isfinite(a) else (float('nan'), float('nan'))
    out = np.array(row, np.float32)
    with np.errstate(all='ignore'):
        xc, zc = np.float64(tx) * c - np.float64(tz) * s, np.float64(tx) * s + np.float64(tz) * c
        x = (PI - np.float64(ry)) + 2.0 * np.float64(a)
        out[3], out[5] = -xc * c + zc * s, xc * s + zc * c
        out[6] = x - 2.0 * PI * np.ceil((x - PI) / (2.0 * PI))
    return out


def view_labels(labels, flip_mask, rot_angle=None):
    """[V, n, 7] fp32 decoded labels -> [V, n, 7] fp32 view labels (the mirrored views brought back)."""
    labels = np.asarray(labels, np.float32)
    out = labels.copy()
    for v in range(len(labels)):
        if (flip_mask >> v) & 1:
            for i in range(labels.shape[1]):
                out[v, i] = unmirror(labels[v, i], 0.0 if rot_angle is None else rot_angle[i])
    return out


def corners_f32(row, tx, yc, tz):
    """[8, 3] fp32 by the fp32 formula of k_detect_decode with the centre (tx, yc, tz): every operation rounded to fp32, no contraction
    (the sine and cosine are the fp64 ones rounded)."""
    f = np.float32
    h, w, l, ry = f(row[0]), f(row[1]), f(row[2]), f(row[6])
    tx, yc, tz = f(tx), f(yc), f(tz)
    cr, sn = f(math.cos(float(ry))), f(math.sin(float(ry)))
    out = np.zeros((8, 3), f)
    with np.errstate(all='ignore'):
        for c in range(8):
            x, y, z = f((-l if c & 2 else l) / f(2)), f((h if c < 4 else -h) / f(2)), f((-w if (c + 1) & 2 else w) / f(2))
            out[c] = (f(f(f(cr * x) + f(sn * z)) + tx), f(y + yc), f(f(f(-sn * x) + f(cr * z)) + tz))
    return out


def label_corners(row):
    f = np.float32
    return corners_f32(row, row[3], f(f(row[4]) - f(f(row[0]) / f(2))), row[5])


def pair_corners(lu, lv):
    """The two corner sets whose IoU is the pair's: box u at translation 0, box v at the fp32 differences of the centres."""
    f = np.float32
    lu, lv = np.asarray(lu, f), np.asarray(lv, f)
    yu, yv = f(lu[4] - f(lu[0] / f(2))), f(lv[4] - f(lv[0] / f(2)))
    return corners_f32(lu, 0, 0, 0), corners_f32(lv, f(lv[3] - lu[3]), f(yv - yu), f(lv[5] - lu[5]))


def pair_iou(lu, lv, iou=None):
    """(iou3d, iou2d) of two view labels, a NaN as 0."""
    k1, k2 = pair_corners(lu, lv)
    v = (iou or FN.iou_corners)(k1.astype(np.float64), k2.astype(np.float64))
    return tuple(0.0 if x != x else float(x) for x in v)


def pairs_of(V):
    return [(u, v) for u in range(V) for v in range(u + 1, V)]


def ensemble(labels, weights, flip_mask=0, rot_angle=None, corners0=None, vote_threshold=0.0, metric=FN.IOU3D, iou=None, views=None):
    """labels [V, n, 7], weights [V, n], corners0 [n, 8, 3] (default: built from labels[0]) -> dict(label_out fp32 [n,7], corners_out fp32
    [n,8,3], agreement fp32 [n], min_iou fp32 [n], anchor int32 [n], n_votes int32 [n], fused {i: rows (w, cx, cy, cz, l', w', h, delta),
    the anchor first, then its voters in view order}, voters {i: [(view, IoU with the anchor)]}, means {i: [mean IoU per valid view]},
    ious {i: {(u, v): IoU}}, views the fp32 view labels [V, n, 7]).  views: view labels computed before (they depend on labels,
    flip_mask and rot_angle only)."""
    labels32 = np.asarray(labels, np.float32)
    V, n = labels32.shape[:2]
    weights = np.asarray(weights, np.float32).reshape(V, n)
    L = view_labels(labels32, flip_mask, rot_angle) if views is None else views
    thr = float(np.float32(vote_threshold))
    if corners0 is None:
        corners0 = np.stack([label_corners(r) for r in labels32[0]]) if n else np.zeros((0, 8, 3), np.float32)
    corners0 = np.asarray(corners0, np.float32).reshape(n, 8, 3)
    out = dict(label_out=labels32[0].copy(), corners_out=corners0.copy(), agreement=np.zeros(n, np.float32), min_iou=np.zeros(n, np.float32),
               anchor=np.full(n, -1, np.int32), n_votes=np.zeros(n, np.int32), fused={}, voters={}, means={}, ious={}, views=L)
    for i in range(n):
        ok = [bool(np.isfinite(L[v, i]).all()) for v in range(V)]
        valid = [v for v in range(V) if ok[v]]
        m = len(valid)
        if m == 0:
            continue
        I = {(u, v): pair_iou(L[u, i], L[v, i], iou)[metric] for u, v in pairs_of(V) if ok[u] and ok[v]}
        out['ious'][i] = I
        if I:
            total = 0.0
            for p in pairs_of(V):
                if p in I:
                    total = total + I[p]
            out['agreement'][i] = np.float32(total / len(I))
            out['min_iou'][i] = np.float32(min(I.values()))
        of = lambda x, y: I[(min(x, y), max(x, y))]
        means = {}
        for v in valid:
            s = 0.0
            for u in valid:
                if u != v:
                    s = s + of(u, v)
            means[v] = s / (m - 1) if m > 1 else 0.0
        a = valid[0]
        for v in valid:
            if means[v] > means[a]:
                a = v
        out['anchor'][i], out['means'][i] = a, means
        lab = L[:, i].astype(np.float64)
        h, w, l, tx, ty, tz, ry = lab[a]
        rows = [(usable(weights[a, i]), tx, ty - h / 2.0, tz, l, w, h, 0.0)]
        voters = []
        for v in valid:
            if v == a or not np.float32(of(a, v)) > np.float32(thr):
                continue
            x = float(np.float32(of(a, v)))               # (the device holds the IoU in fp32; the specification's own value is rounded likewise)
            hv, wv, lv, txv, tyv, tzv, ryv = lab[v]
            k, delta = align(ry, ryv)
            if k & 1:
                lv, wv = wv, lv
            rows.append((usable(weights[v, i]) * x, txv, tyv - hv / 2.0, tzv, lv, wv, hv, delta))
            voters.append((v, of(a, v)))
        out['n_votes'][i], out['voters'][i] = len(voters), voters
        W = 0.0
        for r in rows:
            W = W + r[0]
        if len(rows) == 1 or not (W > 0.0 and math.isfinite(W)):
            if a != 0:
                out['label_out'][i] = L[a, i]
                out['corners_out'][i] = label_corners(L[a, i])
            continue
        s = [0.0] * 7
        for r in rows:
            for c in range(7):
                s[c] = s[c] + r[0] * r[1 + c]
        cx, cy, cz, lf, wf, hf = (s[c] / W for c in range(6))
        out['label_out'][i] = np.asarray([hf, wf, lf, cx, cy + hf / 2.0, cz, ry + s[6] / W], np.float64).astype(np.float32)
        out['corners_out'][i] = label_corners(out['label_out'][i])
        out['fused'][i] = np.asarray(rows, np.float64)
    return out


OUTPUTS = ('label_out', 'corners_out', 'agreement', 'min_iou', 'anchor', 'n_votes')


class DetectEnsembleSpec:
    """Mix-in: t3d_detect_ensemble for a specification library (FakeLib and its subclasses)."""

    def t3d_detect_ensemble(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if p.n < 0 or p.V < 1:
            return -1
        if p.V > MAX_VIEWS:
            return -2
        if p.metric not in (FN.IOU3D, FN.IOU2D) or (p.flip_mask & 1) or (p.flip_mask >> p.V):
            return -1
        if not 0.0 <= p.vote_threshold <= 1.0:
            return -1
        if p.n == 0:
            return 0
        if not all(p.label[v] and p.weight[v] for v in range(p.V)):
            return -1
        if not (p.corners0 and p.label_out and p.corners_out and p.agreement and p.min_iou and p.anchor and p.n_votes):
            return -1
        need = abi.detect_ensemble_workspace_bytes(p.n, p.V)
        if p.workspace_bytes < need or (need and not p.workspace) or (p.workspace or 0) % 8:
            return -1
        n, V = p.n, p.V
        inputs = [arr(p.label[v], n, 7) for v in range(V)] + [arr(p.weight[v], n) for v in range(V)] + [arr(p.corners0, n, 8, 3)]
        rot = arr(p.rot_angle, n) if p.rot_angle else None
        before = [x.copy() for x in inputs]
        out = ensemble(np.stack(inputs[:V]), np.stack(inputs[V:2 * V]), p.flip_mask, rot, inputs[2 * V], p.vote_threshold, p.metric)
        arr(p.label_out, n, 7)[:], arr(p.corners_out, n, 8, 3)[:] = out['label_out'], out['corners_out']
        arr(p.agreement, n)[:], arr(p.min_iou, n)[:], arr(p.anchor, n)[:], arr(p.n_votes, n)[:] = (out[k] for k in OUTPUTS[2:])
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(inputs, before)), 'the outputs overlap an input'
        return 0


class FakeEnsembleLib(DetectEnsembleSpec, FF.FakeFuseLib):
    pass
