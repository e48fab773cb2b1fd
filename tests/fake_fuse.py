"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_detect_fuse (include/t3d.h, csrc/fuse.hip): `fuse_clusters` is
the rule on arrays, DetectFuseSpec the entry point behind the ctypes struct on host pointers, so that nms.DeviceFuse, semisup_infer.
inference(decode='device', nms=NmsRequest(fuse=True)) and transferable3d_amd/detect.py --nms_fuse run end to end through
Runtime(device='cpu', lib=FakeFuseLib())."""
import math

import numpy as np

import fake_nms as FN
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

PI = math.pi


def wrap(x):
    """into (-pi, pi]"""
    return x - 2.0 * PI * math.ceil((x - PI) / (2.0 * PI))


def align(ry_i, ry_j):
    """(k, delta): the quarter turn k in 0..3 that brings heading ry_j nearest to ry_i (the lowest k on a tie) and what is left."""
    best = None
    for k in range(4):
        w = wrap((ry_j - ry_i) + k * (PI / 2.0))
        if best is None or abs(w) < abs(best[1]):
            best = (k, w)
    return best


def usable(w):
    """A weight that is negative, NaN or infinite counts as 0."""
    w = float(w)
    return w if math.isfinite(w) and w >= 0.0 else 0.0


def label_corners_f32(label):
    """[8, 3] fp32 from an fp32 label row (h, w, l, tx, ty, tz, ry) by the fp32 formula of k_detect_decode (csrc/detect.hip): every
    operation rounded to fp32, no contraction."""
    f = np.float32
    h, w, l, tx, ty, tz, ry = (f(v) for v in label)
    cr, sn = f(np.cos(ry)), f(np.sin(ry))
    out = np.zeros((8, 3), f)
    for c in range(8):
        x, y, z = f((-l if c & 2 else l) / f(2)), f((h if c < 4 else -h) / f(2)), f((-w if (c + 1) & 2 else w) / f(2))
        out[c] = (f(f(f(cr * x) + f(sn * z)) + tx), f(y + f(ty - f(h / f(2)))), f(f(f(-sn * x) + f(cr * z)) + tz))
    return out


def fuse_clusters(label, corners, weight, group_offsets, members, keep, suppressed_by, rank, vote_threshold, metric=FN.IOU3D,
                  fill=None, cache=None, iou=None):
    """-> (label_out fp32 [n,7], corners_out fp32 [n,8,3], n_votes int32 [n], clusters).  Boxes in no group hold `fill` = (label value,
    corners value, n_votes value); default: copies of their inputs and 0.  clusters: {anchor: rows (w, cx, cy, cz, l', w', h, delta),
    the anchor first, then its voters in rank order} for every kept box that was fused (what the comparison's bound is made of).
    cache: {(i, j): (iou3d, iou2d)} as fake_nms.group_pairs fills it, read and extended; iou: fake_nms.iou_corners or a memoising one."""
    label32, corners32 = np.asarray(label, np.float32).reshape(-1, 7), np.asarray(corners, np.float32).reshape(-1, 8, 3)
    n = len(label32)
    lab, k64 = label32.astype(np.float64), corners32.astype(np.float64)
    cache, iou = {} if cache is None else cache, iou or FN.iou_corners
    thr = float(np.float32(vote_threshold))
    if fill is None:
        label_out, corners_out, votes = label32.copy(), corners32.copy(), np.zeros(n, np.int32)
    else:
        label_out, corners_out, votes = np.full((n, 7), fill[0], np.float32), np.full((n, 8, 3), fill[1], np.float32), np.full(n, fill[2], np.int32)
    clusters = {}
    for g in range(len(group_offsets) - 1):
        boxes = [int(b) for b in members[group_offsets[g]:group_offsets[g + 1]]]
        order = sorted(boxes, key=lambda b: rank[b])
        for i in boxes:
            label_out[i], corners_out[i] = label32[i], corners32[i]
            if not keep[i]:
                votes[i] = -1
                continue
            votes[i] = 0
            if not np.isfinite(lab[i]).all():
                continue
            h, w, l, tx, ty, tz, ry = lab[i]
            wi = usable(weight[i])
            rows = [(wi, tx, ty - h / 2.0, tz, l, w, h, 0.0)]
            for j in order:
                if j == i or keep[j] or suppressed_by[j] != i or not np.isfinite(lab[j]).all():
                    continue
                if (i, j) not in cache:
                    cache[(i, j)] = iou(k64[i], k64[j])
                v = cache[(i, j)][metric]
                if not v > thr:                                  # (a NaN does not vote)
                    continue
                hj, wj, lj, txj, tyj, tzj, ryj = lab[j]
                k, delta = align(ry, ryj)
                if k & 1:
                    lj, wj = wj, lj
                rows.append((usable(weight[j]) * v, txj, tyj - hj / 2.0, tzj, lj, wj, hj, delta))
            votes[i] = len(rows) - 1
            W = 0.0
            for r in rows:
                W = W + r[0]
            if len(rows) == 1 or not (W > 0.0 and math.isfinite(W)):
                continue
            s = [0.0] * 7
            for r in rows:
                for c in range(7):
                    s[c] = s[c] + r[0] * r[1 + c]
            cx, cy, cz, lf, wf, hf = (s[c] / W for c in range(6))
            label_out[i] = np.asarray([hf, wf, lf, cx, cy + hf / 2.0, cz, ry + s[6] / W], np.float64).astype(np.float32)
            corners_out[i] = label_corners_f32(label_out[i])
            clusters[i] = np.asarray(rows, np.float64)
    return label_out, corners_out, votes, clusters


class DetectFuseSpec:
    """Mix-in: t3d_detect_fuse for a specification library (FakeLib and its subclasses)."""

    def t3d_detect_fuse(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if p.n < 0 or p.n_groups < 0 or p.max_group < 0 or p.metric not in (FN.IOU3D, FN.IOU2D):
            return -1
        if not 0.0 <= p.vote_threshold <= 1.0:
            return -1
        if p.max_group > FN.MAX_GROUP:
            return -2
        if p.n == 0 or p.n_groups == 0 or p.max_group == 0:
            return 0
        if not (p.group_offsets and p.members and p.keep and p.suppressed_by and p.rank and p.label and p.corners and p.weight
                and p.workspace and p.label_out and p.corners_out and p.n_votes):
            return -1
        if p.workspace_bytes < abi.detect_fuse_workspace_bytes(p.n) or p.workspace % 8:
            return -1
        n = p.n
        go = arr(p.group_offsets, p.n_groups + 1).copy()
        assert np.diff(go).max() <= p.max_group, 'a group larger than the caller declared'
        mem = arr(p.members, max(int(go[-1]), 1))[:go[-1]].copy()
        inputs = [arr(p.label, n, 7), arr(p.corners, n, 8, 3), arr(p.weight, n), arr(p.keep, n), arr(p.suppressed_by, n), arr(p.rank, n)]
        before = [x.copy() for x in inputs]
        lo, ko, nv, _ = fuse_clusters(inputs[0], inputs[1], inputs[2], go, mem, inputs[3], inputs[4], inputs[5], p.vote_threshold, p.metric)
        arr(p.label_out, n, 7)[mem], arr(p.corners_out, n, 8, 3)[mem], arr(p.n_votes, n)[mem] = lo[mem], ko[mem], nv[mem]
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(inputs, before)), 'the outputs overlap an input'
        return 0


class FakeFuseLib(DetectFuseSpec, FN.FakeNmsLib):
    pass
