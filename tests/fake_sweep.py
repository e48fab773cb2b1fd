"""TEST INFRASTRUCTURE ONLY -- the executable specification of t3d_detect_nms_sweep and t3d_sunrgbd_eval_sweep (include/t3d.h,
csrc/nms_sweep.hip, csrc/sunrgbd_sweep.hip).  Neither is a second implementation: a configuration's answer is DEFINED as what the
existing specification answers on that configuration alone, so `nms_sweep` calls fake_nms.greedy_nms once per configuration on the
restricted groups and `eval_sweep` calls the evaluation (FakeSunrgbdEvalLib.t3d_sunrgbd_eval, or any library's) once per configuration on
the selected detections.  SweepSpec is the mix-in that puts both behind the ctypes structs on host pointers, so that nms.DeviceNmsSweep,
evaluate_sunrgbd.sweep and detect --sweep run end to end through Runtime(device='cpu', lib=...)."""
import ctypes as C

import numpy as np

import fake_nms as FN
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

MAX_THRESHOLDS, MAX_CONFIGS = 16, 65536


def restricted(group_offsets, members, sel):
    """The lists with every box b of sel[b] == False left out: (group_offsets, members)."""
    groups = [[int(b) for b in members[group_offsets[g]:group_offsets[g + 1]] if sel[b]] for g in range(len(group_offsets) - 1)]
    return (np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32),
            np.asarray([b for g in groups for b in g], np.int32))


def nms_sweep(corners, score, group_offsets, members, thresholds, config_threshold, listed=None, metric=FN.IOU3D, cache=None):
    """-> (keep uint8 [M, n], n_kept int32 [M]).  Row m: greedy_nms into a zero-filled keep, with thresholds[config_threshold[m]] (no
    threshold for -1: nothing exceeds +inf) on the groups restricted to listed[m]; a row whose index names no threshold stays 0."""
    n, M = len(score), len(config_threshold)
    keep = np.zeros((M, n), np.uint8)
    cache = {} if cache is None else cache
    for m in range(M):
        ct = int(config_threshold[m])
        if ct < -1 or ct >= len(thresholds):
            continue
        sel = np.ones(n, bool) if listed is None else np.asarray(listed[m][:n]) != 0
        go, mem = restricted(group_offsets, members, sel)
        keep[m] = FN.greedy_nms(corners, score, go, mem, np.inf if ct < 0 else thresholds[ct], metric, fill=(0, -1, -1), cache=cache)[0]
    return keep, keep.sum(1).astype(np.int32)


def subset_eval_args(p, sel, keepalive):
    """A t3d_sunrgbd_eval argument struct for the detections `sel` (file indices, ascending) of the call `p`, with outputs of its own."""
    P, G, k = len(sel), p.G, keepalive
    def det(ptr, *shape):
        a = np.ascontiguousarray(arr(ptr, p.P, *shape)[sel]) if p.P else np.zeros((0,) + shape)
        k.append(a)
        return a.ctypes.data_as(type(ptr)) if P else type(ptr)()
    def out(T, dtype, n):
        a = np.zeros(max(n, 1), dtype)
        k.append(a)
        return a, a.ctypes.data_as(T)
    ws_bytes = abi.sunrgbd_eval_workspace_bytes(P, G)
    ws = np.zeros(ws_bytes // 8 + 1, np.int64)
    k.append(ws)
    o = {}
    a = abi.SunrgbdEvalArgs(P=P, G=G, det_centroid=det(p.det_centroid, 3), det_basis=det(p.det_basis, 9), det_coeffs=det(p.det_coeffs, 3),
                            det_confidence=det(p.det_confidence), det_image=det(p.det_image), gt_centroid=p.gt_centroid, gt_basis=p.gt_basis,
                            gt_coeffs=p.gt_coeffs, gt_image=p.gt_image, n_images=p.n_images, image_ids=p.image_ids,
                            image_gt_offsets=p.image_gt_offsets, image_gt=p.image_gt, threshold=p.threshold, workspace=ws.ctypes.data,
                            workspace_bytes=ws_bytes)
    for name, T, dt, n in (('order', abi.I, np.int32, P), ('max_overlap', abi.D, np.float64, P), ('gt_idx', abi.I, np.int32, P),
                           ('is_tp', abi.U8, np.uint8, P), ('is_fp', abi.U8, np.uint8, P), ('gt_assignment', abi.I, np.int32, P),
                           ('is_missed', abi.U8, np.uint8, G), ('precision', abi.D, np.float64, P), ('recall', abi.D, np.float64, P),
                           ('ap', abi.D, np.float64, 1)):
        o[name], ptr = out(T, dt, n)
        setattr(a, name, ptr)
    return a, o


def eval_sweep(evaluate, p, mask, det_index=None):
    """evaluate(args struct) -> return code: one class's evaluation (a library's t3d_sunrgbd_eval without the stream).  p: the argument
    struct of the whole class; mask [M, columns]; det_index [P] or None.  -> (ap float64 [M], n_det, n_tp, n_fp int32 [M]): per row the
    evaluation of the selected detections alone."""
    M = len(mask)
    cols = np.arange(p.P) if det_index is None else np.asarray(det_index, np.int64)
    ap, n_det, n_tp, n_fp = np.zeros(M), np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros(M, np.int32)
    for m in range(M):
        row = np.asarray(mask[m])
        ok = (cols >= 0) & (cols < len(row))
        picked = np.zeros(len(cols), bool)
        picked[ok] = row[cols[ok]] != 0                      # (a column outside the row selects nothing)
        sel = np.nonzero(picked)[0]
        keepalive = []
        a, o = subset_eval_args(p, sel, keepalive)
        assert evaluate(a) == 0
        ap[m], n_det[m] = o['ap'][0], len(sel)
        n_tp[m], n_fp[m] = int(o['is_tp'][:len(sel)].sum()), int(o['is_fp'][:len(sel)].sum())
    return ap, n_det, n_tp, n_fp


class SweepSpec:
    """Mix-in: t3d_detect_nms_sweep and t3d_sunrgbd_eval_sweep for a specification library that has t3d_sunrgbd_eval."""

    def t3d_detect_nms_sweep(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if p.n < 0 or p.n_groups < 0 or p.max_group < 0 or p.metric not in (FN.IOU3D, FN.IOU2D):
            return -1
        if p.max_group > FN.MAX_GROUP or not 1 <= p.M <= MAX_CONFIGS or not 1 <= p.n_thresholds <= MAX_THRESHOLDS:
            return -2
        thresholds = [float(p.thresholds[k]) for k in range(p.n_thresholds)]
        if any(t != t for t in thresholds) or not p.n_kept or (p.keep and p.keep_stride < p.n):
            return -1
        n, M = p.n, p.M
        empty = n == 0 or p.n_groups == 0 or p.max_group == 0
        if not empty:
            if not (p.corners and p.score and p.group_offsets and p.members and p.config_threshold and p.keep and p.workspace):
                return -1
            if p.listed and p.listed_stride < n:
                return -1
            if p.workspace_bytes < abi.detect_nms_sweep_workspace_bytes(n, p.max_group, p.n_thresholds) or p.workspace % 8:
                return -1
        arr(p.n_kept, M)[:] = 0
        if p.keep and n:
            arr(p.keep, M, p.keep_stride)[:, :n] = 0
        if empty:
            return 0
        go = arr(p.group_offsets, p.n_groups + 1).copy()
        assert np.diff(go).max() <= p.max_group, 'a group larger than the caller declared'
        mem = arr(p.members, max(int(go[-1]), 1))[:go[-1]].copy()
        listed = arr(p.listed, M, p.listed_stride) if p.listed else None
        keep, n_kept = nms_sweep(arr(p.corners, n, 8, 3), arr(p.score, n), go, mem, thresholds, arr(p.config_threshold, M), listed, p.metric)
        arr(p.keep, M, p.keep_stride)[:, :n] = keep
        arr(p.n_kept, M)[:] = n_kept
        return 0

    def t3d_sunrgbd_eval_sweep(self, a, s, stream):
        try:
            p, q = _struct(a), _struct(s)
        except AbiSizeError:
            return abi.ERR_ABI
        if not (q.ap and q.n_det and q.n_tp and q.n_fp) or p.gt_difficult:
            return -1
        if p.P < 0 or p.G < 0 or not 1 <= q.M <= MAX_CONFIGS:
            return -2
        if p.P > 0 and (not q.mask or q.mask_stride < (1 if q.det_index else p.P)):
            return -1
        if p.G > 0 and (not q.workspace or q.workspace_bytes < abi.sunrgbd_sweep_workspace_bytes(q.M, p.G) or q.workspace % 8):
            return -1
        e = self.t3d_sunrgbd_eval(a, stream)
        if e != 0:
            return e
        mask = arr(q.mask, q.M, q.mask_stride) if p.P else np.zeros((q.M, 0), np.uint8)
        index = arr(q.det_index, p.P).copy() if q.det_index and p.P else None
        out = eval_sweep(lambda sub: self.t3d_sunrgbd_eval(C.byref(sub), stream), p, mask, index)
        for name, v in zip(('ap', 'n_det', 'n_tp', 'n_fp'), out):
            arr(getattr(q, name), q.M)[:] = v
        return 0
