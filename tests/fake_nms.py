"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_detect_nms (include/t3d.h, csrc/nms.hip): `greedy_nms` is the
rule on arrays, DetectNmsSpec the entry point behind the ctypes struct on host pointers, so that nms.DeviceNms, semisup_infer.inference(
decode='device', nms=...) and transferable3d_amd/detect.py --nms_iou run end to end through Runtime(device='cpu', lib=FakeNmsLib())."""
import numpy as np

from fake_detect import DetectDecodeSpec
from fake_t3d import AbiSizeError, FakeLib, _struct, arr, iou_from_quads
from transferable3d_amd import abi

IOU3D, IOU2D = 0, 1
MAX_GROUP = 1024


def iou_corners(k1, k2):
    """(iou3d, iou2d) of two boxes as 8 corners in get_3d_box order, as box3d_iou_corners of csrc/boxgeom_dev.h defines them (the
    arithmetic of fake_t3d.FakeLib.t3d_box3d_iou_corners), in fp64."""
    k1, k2 = np.asarray(k1, np.float64), np.asarray(k2, np.float64)
    vol = lambda k: np.linalg.norm(k[0] - k[1]) * np.linalg.norm(k[1] - k[2]) * np.linalg.norm(k[0] - k[4])
    with np.errstate(invalid='ignore', divide='ignore'):
        i3, i2 = iou_from_quads(k1[[3, 2, 1, 0]][:, [0, 2]], k2[[3, 2, 1, 0]][:, [0, 2]], k1[0, 1], k1[4, 1], k2[0, 1], k2[4, 1], vol(k1), vol(k2))
    return float(i3), float(i2)


def near_matrix(corners):
    """[m, m] bool: False where two boxes' centres are farther apart than the sum of their half diagonals -- they cannot touch, both
    IoUs are exactly 0 and are not computed (a group of 1024 has half a million pairs)."""
    c = corners.mean(1)
    half = 0.5 * np.linalg.norm(corners[:, 0] - corners[:, 6], axis=1)
    dist = np.linalg.norm(c[:, None] - c[None], axis=2)
    return dist <= (half[:, None] + half[None]) * (1 + 1e-9) + 1e-9


def group_order(score, boxes):
    """The boxes of one group, best first: descending score, a NaN as -inf, equal scores by ascending box index."""
    key = np.asarray(score, np.float64)[boxes]
    key = np.where(np.isnan(key), -np.inf, key)
    return [int(boxes[k]) for k in np.lexsort((np.asarray(boxes), -key))]


def group_pairs(corners, score, boxes, cache=None, iou=None):
    """(order, {(i, j): (iou3d, iou2d)}) of one group: every pair of boxes that can touch, the better-ranked box i as the first argument.
    `cache`: a dict that keeps the pairs between calls (other thresholds and metrics on the same boxes); `iou`: iou_corners or a
    function that remembers its answers."""
    cache, iou = {} if cache is None else cache, iou or iou_corners
    order = group_order(score, boxes)
    near = near_matrix(corners[order])
    for a in range(len(order)):
        for b in np.nonzero(near[a, a + 1:])[0] + a + 1:
            key = (order[a], order[b])
            if key not in cache:
                cache[key] = iou(corners[key[0]], corners[key[1]])
    return order, cache


def greedy_nms(corners, score, group_offsets, members, threshold, metric=IOU3D, fill=(1, -1, -1), cache=None):
    """-> (keep uint8 [n], suppressed_by int32 [n], rank int32 [n]); boxes in no group hold `fill`."""
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    n = len(corners)
    keep, sup, rank = np.full(n, fill[0], np.uint8), np.full(n, fill[1], np.int32), np.full(n, fill[2], np.int32)
    thr = float(np.float32(threshold))
    for g in range(len(group_offsets) - 1):
        boxes = np.asarray(members[group_offsets[g]:group_offsets[g + 1]], np.int64)
        order, pairs = group_pairs(corners, score, boxes, cache)
        kept = []
        for r, j in enumerate(order):
            rank[j] = r
            by = next((i for i in kept if pairs.get((i, j), (0.0, 0.0))[metric] > thr), None)      # (a NaN compares false)
            keep[j], sup[j] = (1, -1) if by is None else (0, by)
            if by is None:
                kept.append(j)
    return keep, sup, rank


class DetectNmsSpec:
    """Mix-in: t3d_detect_nms for a specification library (FakeLib and its subclasses)."""

    def t3d_detect_nms(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if p.n < 0 or p.n_groups < 0 or p.max_group < 0 or p.metric not in (IOU3D, IOU2D):
            return -1
        if p.max_group > MAX_GROUP:
            return -2
        if p.n == 0 or p.n_groups == 0 or p.max_group == 0:
            return 0
        if not (p.corners and p.score and p.group_offsets and p.members and p.keep and p.suppressed_by and p.workspace):
            return -1
        if p.workspace_bytes < abi.detect_nms_workspace_bytes(p.n, p.max_group) or p.workspace % 8:
            return -1
        n = p.n
        go = arr(p.group_offsets, p.n_groups + 1).copy()
        assert np.diff(go).max() <= p.max_group, 'a group larger than the caller declared'
        mem = arr(p.members, max(int(go[-1]), 1))[:go[-1]].copy()
        keep, sup, rank = arr(p.keep, n), arr(p.suppressed_by, n), arr(p.rank, n) if p.rank else None
        k, s, r = greedy_nms(arr(p.corners, n, 8, 3), arr(p.score, n), go, mem, p.threshold, p.metric)
        keep[mem], sup[mem] = k[mem], s[mem]
        if rank is not None:
            rank[mem] = r[mem]
        return 0


class FakeNmsLib(DetectNmsSpec, DetectDecodeSpec, FakeLib):
    pass
