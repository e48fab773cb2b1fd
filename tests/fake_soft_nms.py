"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_detect_soft_nms (include/t3d.h, csrc/soft_nms.hip): `soft_nms`
is the rule on arrays, DetectSoftNmsSpec the entry point behind the ctypes struct on host pointers, so that nms.DeviceSoftNms,
semisup_infer.inference(decode='device', nms=NmsRequest(soft=...)) and transferable3d_amd/detect.py --soft_nms run end to end through
Runtime(device='cpu', lib=FakeSoftNmsLib()).

The rule, per group (t3d.h has the same text):
  1 every box starts with its input score; a listed box whose score is not a finite number above 0 takes no part (keep 1, suppressed_by
    -1, score_out the input bits, n_decays 0);
  2 until no box is live, the live box with the largest working score is selected -- on equal scores the lower box index -- and kept;
    its score_out is its working score at that moment;
  3 every box j still live is decayed by IoU(selected, j), the selected box as the first argument: gaussian, IoU > 0: score *=
    exp(-IoU^2 / sigma); linear, IoU > threshold: score *= 1 - IoU; a NaN IoU decays nothing;
  4 a box whose working score falls below min_score (strictly) by a decay is pruned: keep 0, suppressed_by the selected box, score_out
    the value it fell to;
  5 n_decays counts the selected boxes that decayed a box;  6 a box in no group keeps what the outputs held.

`soft_nms` also carries, per box, a bound on how far an implementation that takes its IoUs within `eps` of this one's may land from
score_out (soft_nms_check derives it), and reports the boxes whose decisions could flip inside that bound."""
import math

import numpy as np

from fake_nms import IOU2D, IOU3D, MAX_GROUP, FakeNmsLib, iou_corners, near_matrix
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

GAUSSIAN, LINEAR = 0, 1
ULPS = 8 * 2.0 ** -23            # the fp32 arithmetic of one decay (soft_nms_check: derivation)


class Result:
    """score_out [n] fp64 (a box that took no part or is unlisted: its input score / the fill), keep, suppressed_by, n_decays; bound [n]:
    the absolute bound of module docstring (0: the score is the input's, bit for bit); unsafe: the boxes whose decisions could flip
    inside twice the bound; slivers: the boxes a gaussian decay met with 0 < IoU < eps -- whether such a pair decays at all is decided
    inside the IoU error (soft_nms_check builds its gaussian cases without them)."""

    def __init__(self, score_out, keep, suppressed_by, n_decays, bound, unsafe, slivers):
        self.score_out, self.keep, self.suppressed_by, self.n_decays = score_out, keep, suppressed_by, n_decays
        self.bound, self.unsafe, self.slivers = bound, unsafe, slivers


def soft_nms(corners, score, group_offsets, members, method, threshold=None, sigma=0.5, min_score=0.001, metric=IOU3D, fill=None,
             cache=None, iou=None, eps=0.0):
    """-> Result.  method GAUSSIAN / LINEAR (or their names); fill: (score_out, keep, suppressed_by, n_decays) of a box in no group
    (default: its input score, 1, -1, 0).  cache: a dict (selected, other) -> (iou3d, iou2d) kept between calls; iou: iou_corners or a
    function that remembers its answers.  eps: the IoU error the bound is accumulated for."""
    method = {'gaussian': GAUSSIAN, 'linear': LINEAR}.get(method, method)
    assert method in (GAUSSIAN, LINEAR)
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    score = np.asarray(score, np.float32)
    n = len(corners)
    cache, iou = {} if cache is None else cache, iou or iou_corners
    out = score.astype(np.float64) if fill is None else np.full(n, fill[0], np.float64)
    fk, fs, fd = (1, -1, 0) if fill is None else fill[1:]
    keep, sup, dec = np.full(n, fk, np.uint8), np.full(n, fs, np.int32), np.full(n, fd, np.int32)
    bound = np.zeros(n)
    unsafe, slivers = set(), set()
    thr = float(np.float32(0.0 if threshold is None else threshold))
    sig, floor = float(np.float32(sigma)), float(np.float32(min_score))
    for g in range(len(group_offsets) - 1):
        boxes = [int(b) for b in members[group_offsets[g]:group_offsets[g + 1]]]
        if not boxes:
            continue
        local = {b: k for k, b in enumerate(boxes)}
        near = near_matrix(corners[boxes])
        for b in boxes:
            out[b], keep[b], sup[b], dec[b] = float(score[b]), 1, -1, 0
        live = [b for b in boxes if math.isfinite(score[b]) and score[b] > 0]
        while live:
            sel = min(live, key=lambda b: (-out[b], b))
            live.remove(sel)
            for j in list(live):
                if not near[local[sel], local[j]]:
                    continue
                if (sel, j) not in cache:
                    cache[(sel, j)] = iou(corners[sel], corners[j])
                v = cache[(sel, j)][metric]
                if method == GAUSSIAN:
                    if not v > 0.0:                     # (a NaN compares false)
                        continue
                    if v < eps:
                        slivers.add(j)
                    f = math.exp(-v * v / sig)
                    df = f * (2.0 * v * eps + eps * eps) / sig
                else:
                    if not v > thr:
                        continue
                    f, df = 1.0 - v, eps
                if abs(out[sel] - out[j]) < 2.0 * (bound[sel] + bound[j]):      # which of the two is selected could flip
                    unsafe.add(j)
                new = out[j] * f
                bound[j] = bound[j] * f + out[j] * df + ULPS * abs(new)
                out[j] = new
                dec[j] += 1
                if abs(new - floor) < 2.0 * bound[j]:                           # whether it is pruned could flip
                    unsafe.add(j)
                if new < floor:
                    live.remove(j)
                    keep[j], sup[j] = 0, sel
    return Result(out, keep, sup, dec, bound, unsafe, slivers)


class DetectSoftNmsSpec:
    """Mix-in: t3d_detect_soft_nms for a specification library (FakeLib and its subclasses)."""

    def t3d_detect_soft_nms(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if p.n < 0 or p.n_groups < 0 or p.max_group < 0 or p.metric not in (IOU3D, IOU2D) or p.method not in (GAUSSIAN, LINEAR):
            return -1
        if p.method == GAUSSIAN and not (p.sigma > 0 and math.isfinite(p.sigma)):
            return -1
        if not p.min_score >= 0:
            return -1
        if p.max_group > MAX_GROUP:
            return -2
        if p.n == 0 or p.n_groups == 0 or p.max_group == 0:
            return 0
        if not (p.corners and p.score and p.group_offsets and p.members and p.score_out and p.keep and p.suppressed_by and p.n_decays):
            return -1
        if p.workspace_bytes < abi.detect_soft_nms_workspace_bytes(p.n, p.max_group):
            return -1
        n = p.n
        go = arr(p.group_offsets, p.n_groups + 1).copy()
        assert np.diff(go).max() <= p.max_group, 'a group larger than the caller declared'
        mem = arr(p.members, max(int(go[-1]), 1))[:go[-1]].copy()
        score = arr(p.score, n).copy()
        r = soft_nms(arr(p.corners, n, 8, 3), score, go, mem, p.method, p.threshold, p.sigma, p.min_score, p.metric)
        out, keep, sup, dec = arr(p.score_out, n), arr(p.keep, n), arr(p.suppressed_by, n), arr(p.n_decays, n)
        new = r.score_out.astype(np.float32)
        same = mem[r.n_decays[mem] == 0]                                         # nothing decayed them: the input bits
        new.view(np.uint32)[same] = score.view(np.uint32)[same]
        out.view(np.uint32)[mem] = new.view(np.uint32)[mem]
        keep[mem], sup[mem], dec[mem] = r.keep[mem], r.suppressed_by[mem], r.n_decays[mem]
        return 0


class FakeSoftNmsLib(DetectSoftNmsSpec, FakeNmsLib):
    pass
