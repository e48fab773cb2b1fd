#!/usr/bin/env python3
"""The official SUN-RGBD 3-D detection AP on the device: evaluation/sunrgbd/detection/script_3Deval.m of the reference without MATLAB.

    python -m transferable3d_amd.evaluate_sunrgbd --pred_dir D --dataset_dir mysunrgbd --idx_path val_data_idx.txt --test_on B
    python -m transferable3d_amd.evaluate_sunrgbd --official_eval --dataset_dir mysunrgbd --idx_path val_data_idx.txt --test_on AB \
        --semi_type F --model_path M --data_path frustums/val.zip.pickle ...          # every other flag is test_semisup's

The second form runs test_semisup's inference on a frustum file and scores the predictions it holds in memory (no text round trip).

`--pred_dir` holds the `<class>_pred.txt` files test_semisup --result_dir (or the reference) writes.  Per class the script's chain
parse_class_predictions -> benchmark_groundtruth -> computePRCurve3D (bb3dOverlapCloseForm, get_average_precision) runs as ONE
t3d_sunrgbd_eval call (csrc/sunrgbd_eval.hip): footprints, the stable order of the confidences, overlaps with the ground truth of the
same image, assignment, precision / recall and AP, all fp64 on the device, one copy back.  The lines printed are the script's.

Ground truth: the toolbox's Metadata/groundtruth.mat is replaced by the label files of the data set directory sunrgbd_data.py reads
(<dataset_dir>/training/label_dimension/%06d.txt): centroid as stored, coeffs (l, w, h) (the file stores half sizes), basis rows
(o1, o2, 0)/|o|, (-o2, o1, 0)/|o|, (0, 0, 1) -- the rectangle sunrgbd_data.compute_box_3d builds.  imageNum is the file's number.

Two deliberate differences from the script: an empty prediction file counts as zero predictions (importdata stops the script there),
and two boxes that both have zero volume overlap by 0 (MATLAB: 0 / 0).

--diagnose [--diagnose_bg 0.1] [--diagnose_json FILE] (either form): why the AP is what it is.  Per class ONE t3d_sunrgbd_diagnose call
(csrc/sunrgbd_diagnose.hip) in place of the t3d_sunrgbd_eval call: the same evaluation, then every false positive sorted into a kind
(cls: on a box of another evaluated class; loc: on its own box, too loose; both; dup: its box was already claimed; bkg), every
missed box into localised or not, and the AP the class would have if each kind of error were fixed -- the breakdown of Bolya et al.,
"TIDE" (ECCV 2020) under this protocol's overlap, matching and AP (include/t3d.h has the rules).  Two lines per class follow its AP line
and one the mean; without the flag nothing changes.

--diagnose --diagnose_parts: which part of a loose box is loose.  Per class ONE t3d_sunrgbd_locparts call (csrc/sunrgbd_locparts.hip) in
place of the t3d_sunrgbd_diagnose call: the same diagnosis, then per detection the overlap with its box once its xy, its z, its centre,
its size or its heading is the box's own, the six errors behind them (centre distance, dz, log size ratios, heading), and the AP the
class would have if every LOC detection that one part repairs were repaired.  Two more lines per class (`Localisation for X:`, `dAP(loc)
for X:`) and `Mean dAP(loc):`.  The parts do not add up: a detection may be repaired by several parts, or only by the centre as a whole.

`sweep_class` / `sweep` (t3d_sunrgbd_eval_sweep, csrc/sunrgbd_sweep.hip): the evaluation of one class for many subsets of its detections in
one call -- footprints, ranks and overlaps once, the claims and the curve per subset -- which `detect --sweep` (sweep.py) scores a grid of
post-processing thresholds with.

--bootstrap R [--bootstrap_seed 0] [--bootstrap_level 0.95] [--bootstrap_json FILE] (either form): how far each AP moves when the image
list is redrawn -- the percentile bootstrap over images (bootstrap.py).  Per class ONE t3d_sunrgbd_eval_bootstrap call
(csrc/sunrgbd_bootstrap.hip) in place of the t3d_sunrgbd_eval call: the same evaluation, then the AP of every redraw from the same
matching with integer weights (`bootstrap_class`).  One `AP interval` line follows each AP line and one `Mean AP interval` line the mean.
--pred_dir A --compare_pred_dir B --bootstrap R (`compare`) scores two directories with the same redraws and prints, per class and for
the mean, `dAP for X (B - A): mean [lo, hi], p(≤0) share`.  --diagnose does not go with it; without the flag nothing changes.
"""
import argparse
import ctypes as C
import json
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import abi
from . import sunrgbd_data as SD

# script_3Deval.m:20-22
CLASS_NAMES = {'A': ['bed', 'chair', 'toilet', 'desk', 'bathtub'],
               'B': ['table', 'sofa', 'dresser', 'night_stand', 'bookshelf'],
               'AB': ['bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub']}
EPS = 2.0 ** -52


def boxes_from_label_format(img_ids, h, w, l, tx, ty, tz, ry, score):
    """parse_class_predictions.m:24-44 on arrays: coeffs (l, w, h) / 2, centroid (tx, tz, h/2 - ty), basis rotz(deg(-ry))',
    confidence = score."""
    h, w, l, tx, ty, tz, ry, score = [np.asarray(v, np.float64).reshape(-1) for v in (h, w, l, tx, ty, tz, ry, score)]
    n = len(h)
    c, s = np.cos(ry), np.sin(ry)
    basis = np.zeros((n, 3, 3))
    basis[:, 0, 0], basis[:, 0, 1] = c, -s
    basis[:, 1, 0], basis[:, 1, 1] = s, c
    basis[:, 2, 2] = 1.0
    return {'centroid': np.stack([tx, tz, h / 2.0 - ty], 1).reshape(n, 3), 'basis': basis,
            'coeffs': np.stack([l / 2.0, w / 2.0, h / 2.0], 1).reshape(n, 3), 'confidence': score,
            'image': np.asarray(img_ids, np.int64).reshape(-1).astype(np.int32)}


def parse_class_predictions(path, classname=None):
    """parse_class_predictions.m: every line `img_id cls -1 -1 -10 box2d(4) h w l tx ty tz ry score` of the file (the class column is
    not looked at, as in the script) -> {'centroid' [P,3], 'basis' [P,3,3], 'coeffs' [P,3], 'confidence' [P], 'image' [P]}.  The
    decimal strings are converted with correct rounding."""
    if not os.path.exists(path):
        raise FileNotFoundError('no prediction file for class %s: %s' % (classname or os.path.basename(path).replace('_pred.txt', ''), path))
    ids, rows = [], []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if len(t) != 17:
                raise ValueError('%s: a prediction line has 17 fields, got %d: %r' % (path, len(t), line))
            ids.append(int(t[0]))
            rows.append([float(v) for v in t[2:]])
    d = np.asarray(rows, np.float64).reshape(-1, 15)
    return boxes_from_label_format(ids, d[:, 7], d[:, 8], d[:, 9], d[:, 10], d[:, 11], d[:, 12], d[:, 13], d[:, 14])


def boxes_from_label_objects(objects, image_ids):
    """Ground-truth boxes from SUNObject3d label lines (see the module text)."""
    n = len(objects)
    basis = np.zeros((n, 3, 3))
    for i, o in enumerate(objects):
        o1, o2 = o.orientation[0], o.orientation[1]
        nrm = math.sqrt(o1 * o1 + o2 * o2)
        basis[i] = [[o1 / nrm, o2 / nrm, 0.0], [-o2 / nrm, o1 / nrm, 0.0], [0.0, 0.0, 1.0]]
    return {'centroid': np.array([o.centroid for o in objects], np.float64).reshape(n, 3), 'basis': basis,
            'coeffs': np.array([[o.l, o.w, o.h] for o in objects], np.float64).reshape(n, 3),
            'image': np.asarray(image_ids, np.int64).reshape(-1).astype(np.int32), 'classname': [o.classname for o in objects]}


def select_boxes(boxes, keep):
    keep = np.asarray(keep)
    out = {k: np.asarray(v)[keep] for k, v in boxes.items() if k != 'classname'}
    if 'classname' in boxes:
        idx = np.nonzero(keep)[0] if keep.dtype == bool else keep
        out['classname'] = [boxes['classname'][int(i)] for i in idx]
    return out


def benchmark_groundtruth(dataset_dir, idx_list, classname=None, workers=SD.MAX_WORKERS):
    """benchmark_groundtruth.m on the label files: the ground truth (of one class, or of all) of the test images `idx_list` (ids, or the
    path of an index file), in image order then line order; the files are read once by a pool of at most sunrgbd_data.MAX_WORKERS
    threads."""
    if isinstance(idx_list, str):
        idx_list = [int(line.rstrip()) for line in open(idx_list) if line.strip()]
    dataset = SD.sunrgbd_object(dataset_dir)
    with ThreadPoolExecutor(max_workers=max(1, min(int(workers), SD.MAX_WORKERS))) as pool:
        per_image = list(pool.map(dataset.get_label_objects, idx_list))
    objects = [o for objs in per_image for o in objs]
    ids = [i for i, objs in zip(idx_list, per_image) for _ in objs]
    gt = boxes_from_label_objects(objects, ids)
    if classname is not None:
        gt = select_boxes(gt, np.array([c == classname for c in gt['classname']], bool))
    return gt


def get_average_precision(precision, recall):
    """get_average_precision.m:15-23 (VOC2011): sentinels, running maximum of the precision from the right, area over the recall steps.
    MATLAB's max(a, b) ignores a NaN, as np.fmax does."""
    mrec = np.concatenate([[0.0], np.asarray(recall, np.float64).reshape(-1), [1.0]])
    mpre = np.concatenate([[0.0], np.asarray(precision, np.float64).reshape(-1), [0.0]])
    for ii in range(len(mpre) - 2, -1, -1):
        mpre[ii] = np.fmax(mpre[ii], mpre[ii + 1])
    ii = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    return float(np.sum((mrec[ii] - mrec[ii - 1]) * mpre[ii]))


def _runtime(rt):
    if rt is not None:
        return rt
    from .engine import Runtime
    return Runtime()


class _Packed:
    """Arrays laid out in one byte buffer (8-byte aligned fields): one copy to the device, or one copy back."""

    def __init__(self):
        self.fields, self.size = {}, 0

    def add(self, name, dtype, n):
        self.fields[name] = (self.size, np.dtype(dtype), int(n))
        self.size += (int(n) * np.dtype(dtype).itemsize + 7) // 8 * 8

    def view(self, host, name):
        off, dt, n = self.fields[name]
        return host[off:off + n * dt.itemsize].view(dt)


def _by_image(img):
    """Boxes grouped by image: (image_ids ascending and distinct, offsets [n + 1], list: ascending index inside an image)."""
    lst = np.argsort(img, kind='stable').astype(np.int32)
    ids, first = np.unique(img[lst], return_index=True)
    return ids, np.concatenate([first, [len(img)]]).astype(np.int32), lst


def _eval_call(det, gt, difficult, threshold, rt, want_overlaps=False, other=None, bg_threshold=None, parts=False):
    """One t3d_sunrgbd_eval call on one class -> host arrays of every output.  other (boxes of the other evaluated classes) and
    bg_threshold: one t3d_sunrgbd_diagnose call instead, the diagnosis' outputs beside the evaluation's; with parts one
    t3d_sunrgbd_locparts call, the split of the localisation errors beside both.  Either way one copy to the device and one copy back."""
    launch, fetch = _eval_prepare(det, gt, difficult, threshold, rt, want_overlaps, other, bg_threshold, parts=parts)
    launch()
    return fetch()


def _eval_prepare(det, gt, difficult, threshold, rt, want_overlaps=False, other=None, bg_threshold=None, sweep=None, boot=None, parts=False):
    """_eval_call in its three steps: packs and uploads the inputs (the one copy to the device) -> (launch: the entry point's launches
    on the runtime's stream, fetch: the one copy back as host arrays).  tools/bench_sunrgbd_diagnose.py times `launch` alone.
    sweep: (mask uint8 [M, stride] on the runtime's device, det_index [P] or None): one t3d_sunrgbd_eval_sweep call instead, and `fetch`
    copies back its four [M] arrays alone ('ap', 'n_det', 'n_tp', 'n_fp').
    boot: (bootstrap.Weights, det_col [P], gt_col [G]): one t3d_sunrgbd_eval_bootstrap call instead, and `fetch` returns the evaluation's
    arrays plus 'boot': {'ap' float64 [R], 'n_pos', 'n_tp', 'n_fp' int64 [R]} (a second copy back).
    parts (with other): one t3d_sunrgbd_locparts call instead of the t3d_sunrgbd_diagnose call, and `fetch` returns 'part_overlap' [P * 5],
    'loc_error' [P * 6], 'ap_part', 'part_counts' and 'part_boxes' [5] as well."""
    rt = _runtime(rt)
    if parts and other is None:
        raise ValueError('the split of the localisation errors belongs to a diagnosis: parts needs other')
    P, G = len(det['confidence']), len(gt['image'])
    gimg = np.asarray(gt['image'], np.int32)
    image_ids, offsets, image_gt = _by_image(gimg)
    n_img = len(image_ids)
    dimg = np.asarray(det['image'], np.int32)
    inp = _Packed()
    host_in = {'det_centroid': (np.float64, det['centroid']), 'det_basis': (np.float64, det['basis']), 'det_coeffs': (np.float64, det['coeffs']),
               'det_confidence': (np.float64, det['confidence']), 'gt_centroid': (np.float64, gt['centroid']), 'gt_basis': (np.float64, gt['basis']),
               'gt_coeffs': (np.float64, gt['coeffs']), 'det_image': (np.int32, dimg), 'gt_image': (np.int32, gimg),
               'image_ids': (np.int32, image_ids), 'image_gt_offsets': (np.int32, offsets), 'image_gt': (np.int32, image_gt)}
    if difficult is not None:
        difficult = np.asarray(difficult).reshape(-1)
        if len(difficult) != G:
            raise ValueError('inconsistent difficulty size.')               # computePRCurve3D.m:3
        host_in['gt_difficult'] = (np.uint8, (difficult != 0))
    if want_overlaps:
        k = np.searchsorted(image_ids, dimg)
        hit = (k < n_img) & (image_ids[np.minimum(k, max(n_img - 1, 0))] == dimg) if n_img else np.zeros(P, bool)
        cnt = np.where(hit, (offsets[1:] - offsets[:-1])[np.minimum(k, max(n_img - 1, 0))], 0) if n_img else np.zeros(P, np.int64)
        ov_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        host_in['overlap_offsets'] = (np.int64, ov_off)
    if sweep is not None and sweep[1] is not None:
        if len(sweep[1]) != P:
            raise ValueError('%d detections, %d columns in det_index' % (P, len(sweep[1])))
        host_in['det_index'] = (np.int32, sweep[1])
    if boot is not None:
        if len(boot[1]) != P or len(boot[2]) != G:
            raise ValueError('%d detections and %d boxes, %d and %d weight columns' % (P, G, len(boot[1]), len(boot[2])))
        host_in['det_col'], host_in['gt_col'] = (np.int32, boot[1]), (np.int32, boot[2])
    if other is not None:
        Go = len(other['image'])
        oimg = np.asarray(other['image'], np.int32)
        other_ids, other_offsets, other_list = _by_image(oimg)
        host_in.update({'other_centroid': (np.float64, other['centroid']), 'other_basis': (np.float64, other['basis']),
                        'other_coeffs': (np.float64, other['coeffs']), 'other_image': (np.int32, oimg), 'other_image_ids': (np.int32, other_ids),
                        'other_image_offsets': (np.int32, other_offsets), 'other_image_list': (np.int32, other_list)})
    for name, (dt, a) in host_in.items():
        inp.add(name, dt, np.asarray(a).size)
    buf = np.zeros(max(inp.size, 8), np.uint8)
    for name, (dt, a) in host_in.items():
        inp.view(buf, name)[:] = np.ascontiguousarray(a, dt).reshape(-1)
    out = _Packed()
    for name, dt, n in (('max_overlap', np.float64, P), ('precision', np.float64, P), ('recall', np.float64, P), ('ap', np.float64, 1),
                        ('order', np.int32, P), ('gt_idx', np.int32, P), ('gt_assignment', np.int32, P), ('is_tp', np.uint8, P),
                        ('is_fp', np.uint8, P), ('is_missed', np.uint8, G)):
        out.add(name, dt, n)
    if other is not None:
        for name, dt, n in (('other_overlap', np.float64, P), ('ap_fixed', np.float64, len(abi.DIAG_FIXES)), ('other_gt', np.int32, P),
                            ('counts', np.int32, len(abi.DIAG_KINDS)), ('gt_counts', np.int32, 3), ('kind', np.uint8, P), ('gt_state', np.uint8, G)):
            out.add(name, dt, n)
    if parts:
        for name, dt, n in (('part_overlap', np.float64, P * len(abi.LOC_PARTS)), ('loc_error', np.float64, P * len(abi.LOC_ERRORS)),
                            ('ap_part', np.float64, len(abi.LOC_PARTS)), ('part_counts', np.int32, len(abi.LOC_PARTS)),
                            ('part_boxes', np.int32, len(abi.LOC_PARTS))):
            out.add(name, dt, n)
    if want_overlaps:
        n_ov = int(ov_off[-1])
        out.add('overlaps', np.float64, n_ov)
        out.add('overlap_gt', np.int32, n_ov)
    dev = rt.device
    d_in = torch.from_numpy(buf).to(dev)
    # zeros, not empty: with P == 0 or G == 0 the entry point leaves the arrays of that length-0 side alone, and the padding between
    # the packed fields travels back to the host
    d_out = torch.zeros(max(out.size, 8), dtype=torch.uint8, device=dev)
    ws_bytes = abi.sunrgbd_eval_workspace_bytes(P, G)
    d_ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)      # every field is written before it is read

    def ptr(base, pk, name, T):
        if name not in pk.fields or pk.fields[name][2] == 0:
            return C.cast(C.c_void_p(0), C.POINTER(T))
        return C.cast(C.c_void_p(base.data_ptr() + pk.fields[name][0]), C.POINTER(T))
    i_, o_ = (lambda n, T: ptr(d_in, inp, n, T)), (lambda n, T: ptr(d_out, out, n, T))
    dbl, i32, u8 = C.c_double, C.c_int32, C.c_uint8
    a = abi.SunrgbdEvalArgs(P, G, i_('det_centroid', dbl), i_('det_basis', dbl), i_('det_coeffs', dbl), i_('det_confidence', dbl),
                            i_('det_image', i32), i_('gt_centroid', dbl), i_('gt_basis', dbl), i_('gt_coeffs', dbl), i_('gt_image', i32),
                            i_('gt_difficult', u8), n_img, i_('image_ids', i32), i_('image_gt_offsets', i32), i_('image_gt', i32),
                            float(threshold), C.c_void_p(d_ws.data_ptr()), ws_bytes, o_('order', i32), o_('max_overlap', dbl),
                            o_('gt_idx', i32), o_('is_tp', u8), o_('is_fp', u8), o_('gt_assignment', i32), o_('is_missed', u8),
                            o_('precision', dbl), o_('recall', dbl), o_('ap', dbl), i_('overlap_offsets', C.c_int64),
                            o_('overlaps', dbl), o_('overlap_gt', i32))
    if want_overlaps and int(ov_off[-1]) == 0:
        a.overlaps, a.overlap_gt = None, None
    held = [d_in, d_out, d_ws]                 # what the argument structs point into lives as long as `launch` does
    if sweep is not None:
        mask = sweep[0]
        M = int(mask.shape[0])
        assert mask.dtype == torch.uint8 and mask.dim() == 2 and (mask.shape[1] <= 1 or mask.stride(1) == 1)
        sw = _Packed()
        for name, dt in (('ap', np.float64), ('n_det', np.int32), ('n_tp', np.int32), ('n_fp', np.int32)):
            sw.add(name, dt, M)
        d_sw = torch.zeros(max(sw.size, 8), dtype=torch.uint8, device=dev)
        sws_bytes = abi.sunrgbd_sweep_workspace_bytes(M, G)
        d_sws = torch.empty((sws_bytes + 7) // 8, dtype=torch.int64, device=dev)
        w_ = lambda n, T: ptr(d_sw, sw, n, T)
        s = abi.SunrgbdSweepArgs(M, abi.u8ptr(mask), i_('det_index', i32), int(mask.stride(0)) if M > 1 and mask.shape[1] > 0 else int(mask.shape[1]),
                                 C.c_void_p(d_sws.data_ptr()), sws_bytes, w_('ap', dbl), w_('n_det', i32), w_('n_tp', i32), w_('n_fp', i32))
        held += [d_sw, d_sws, mask]

        def launch(held=held):
            abi.check(rt.lib.t3d_sunrgbd_eval_sweep(C.byref(a), C.byref(s), rt.stream()), 't3d_sunrgbd_eval_sweep')

        def fetch(held=held, evaluation=False):
            host = d_sw.cpu().numpy()                                       # the one copy back (synchronises)
            res = {name: sw.view(host, name).copy() for name in sw.fields}
            if evaluation:                                                  # (the tests: what t3d_sunrgbd_eval itself wrote, a second copy)
                host = d_out.cpu().numpy()
                res['evaluation'] = {name: out.view(host, name).copy() for name in out.fields}
            return res
        return launch, fetch
    if boot is not None:
        weights = boot[0]
        R = weights.R
        bo = _Packed()
        for name, dt in (('ap', np.float64), ('n_pos', np.int64), ('n_tp', np.int64), ('n_fp', np.int64)):
            bo.add(name, dt, R)
        d_bo = torch.zeros(bo.size, dtype=torch.uint8, device=dev)
        bws_bytes = abi.sunrgbd_bootstrap_workspace_bytes(P)
        d_bws = torch.empty((bws_bytes + 7) // 8, dtype=torch.int64, device=dev)
        b_ = lambda n, T: ptr(d_bo, bo, n, T)
        b = abi.SunrgbdBootstrapArgs(R, abi.iptr(weights.matrix), weights.stride, i_('det_col', i32), i_('gt_col', i32), C.c_void_p(d_bws.data_ptr()),
                                     bws_bytes, b_('ap', dbl), b_('n_pos', C.c_int64), b_('n_tp', C.c_int64), b_('n_fp', C.c_int64))
        held += [d_bo, d_bws, weights]

        def launch(held=held):
            abi.check(rt.lib.t3d_sunrgbd_eval_bootstrap(C.byref(a), C.byref(b), rt.stream()), 't3d_sunrgbd_eval_bootstrap')

        def fetch(held=held):
            host = d_out.cpu().numpy()                                      # (synchronises)
            res = {name: out.view(host, name).copy() for name in out.fields}
            host = d_bo.cpu().numpy()
            res['boot'] = {name: bo.view(host, name).copy() for name in bo.fields}
            return res
        return launch, fetch
    if other is None:
        def launch(held=held):
            abi.check(rt.lib.t3d_sunrgbd_eval(C.byref(a), rt.stream()), 't3d_sunrgbd_eval')
    else:
        dws_bytes = abi.sunrgbd_diagnose_workspace_bytes(P, G, Go)
        d_dws = torch.empty((dws_bytes + 7) // 8, dtype=torch.int64, device=dev)
        d = abi.SunrgbdDiagnoseArgs(Go, i_('other_centroid', dbl), i_('other_basis', dbl), i_('other_coeffs', dbl), i_('other_image', i32),
                                    len(other_ids), i_('other_image_ids', i32), i_('other_image_offsets', i32), i_('other_image_list', i32),
                                    float(bg_threshold), C.c_void_p(d_dws.data_ptr()), dws_bytes, o_('other_overlap', dbl), o_('other_gt', i32),
                                    o_('kind', u8), o_('gt_state', u8), o_('counts', i32), o_('gt_counts', i32), o_('ap_fixed', dbl))
        held.append(d_dws)
        if parts:
            pws_bytes = abi.sunrgbd_locparts_workspace_bytes(P, G)
            d_pws = torch.empty((pws_bytes + 7) // 8, dtype=torch.int64, device=dev)
            q = abi.SunrgbdLocPartsArgs(0, C.c_void_p(d_pws.data_ptr()), pws_bytes, o_('part_overlap', dbl), o_('loc_error', dbl),
                                        o_('part_counts', i32), o_('part_boxes', i32), o_('ap_part', dbl))
            held.append(d_pws)

            def launch(held=held):
                abi.check(rt.lib.t3d_sunrgbd_locparts(C.byref(a), C.byref(d), C.byref(q), rt.stream()), 't3d_sunrgbd_locparts')
        else:
            def launch(held=held):
                abi.check(rt.lib.t3d_sunrgbd_diagnose(C.byref(a), C.byref(d), rt.stream()), 't3d_sunrgbd_diagnose')

    def fetch(held=held):
        host = d_out.cpu().numpy()                                          # the one copy back (synchronises)
        res = {name: out.view(host, name).copy() for name in out.fields}
        if want_overlaps:
            res['overlap_offsets'] = ov_off
        return res
    return launch, fetch


def compute_pr_curve_3d(classname, det, gt, difficult=None, threshold=0.25, rt=None):
    """computePRCurve3D.m with its output names.  `gt` may hold several classes ('classname' per box): the boxes of `classname` are
    picked (:11-14) and isMissed / gtAssignment refer to the whole list, as in the script.  isTp, isFp, gtAssignment are in file order;
    precision, recall, maxOverlaps, gtIdxAll in sorted order (sortIdx, 0-based: sorted position -> file index), as the script leaves them."""
    G_all = len(gt['image'])
    if difficult is None:
        difficult = np.zeros(G_all, np.uint8)
    difficult = np.asarray(difficult).reshape(-1)
    if len(difficult) != G_all:
        raise ValueError('inconsistent difficulty size.')
    same = np.array([c == classname for c in gt['classname']], bool) if 'classname' in gt else np.ones(G_all, bool)
    return _pr_curve_result(_eval_call(det, select_boxes(gt, same), difficult[same], threshold, rt), same)


def _pr_curve_result(r, same):
    """compute_pr_curve_3d's dictionary from the arrays of one call; same: the boxes of the whole ground-truth list that took part."""
    G_all, sel = len(same), np.nonzero(same)[0]
    order = r['order'].astype(np.int64)
    is_missed = np.zeros(G_all, bool)
    is_missed[sel] = r['is_missed'] != 0
    ga = r['gt_assignment'].astype(np.int64)
    ga[ga > 0] = sel[ga[ga > 0] - 1] + 1                                     # tmp = find(isSameClass)  (:47-48)
    return {'apScore': float(r['ap'][0]), 'precision': r['precision'], 'recall': r['recall'], 'isTp': r['is_tp'] != 0, 'isFp': r['is_fp'] != 0,
            'isMissed': is_missed, 'gtAssignment': ga, 'maxOverlaps': r['max_overlap'][order], 'numOfgt': int(same.sum()),
            'gtIdxAll': r['gt_idx'][order].astype(np.int64), 'sortIdx': order}


def sweep_class(classname, det, gt_all, masks, det_index=None, threshold=0.25, rt=None):
    """compute_pr_curve_3d(classname, det', gt_all) for M subsets det' of the detections in one t3d_sunrgbd_eval_sweep call
    (csrc/sunrgbd_sweep.hip): footprints, ranks and overlaps once, then the claims and the curve of every subset.  masks: uint8
    [M, >= columns], NumPy (uploaded) or a tensor on the runtime's device -- the `keep` matrix of nms.DeviceNmsSweep as it lies;
    det_index [P]: the column of detection i (None: i).  Subset m holds the detections whose column of row m is not 0, in file order.
    -> {'ap' float64 [M], 'n_det', 'n_tp', 'n_fp' int32 [M]}: one upload of the class (plus the masks, where they come from the host)
    and one copy back of the four arrays."""
    rt = _runtime(rt)
    same = np.array([c == classname for c in gt_all['classname']], bool) if 'classname' in gt_all else np.ones(len(gt_all['image']), bool)
    if not torch.is_tensor(masks):
        masks = torch.from_numpy(np.ascontiguousarray(np.asarray(masks) != 0, np.uint8)).to(rt.device)
    if masks.dim() != 2 or not 1 <= masks.shape[0] <= abi.SWEEP_MAX_CONFIGS:
        raise ValueError('masks is [M, columns] with 1 <= M <= %d' % abi.SWEEP_MAX_CONFIGS)
    launch, fetch = _eval_prepare(det, select_boxes(gt_all, same), None, threshold, rt, sweep=(masks, det_index))
    launch()
    return fetch()


def sweep(predictions, dataset_dir, idx_list, masks, det_index, test_on='AB', rt=None, threshold=0.25, gt_all=None):
    """sweep_class over the classes of the set `test_on`: predictions {class: boxes} as `evaluate` takes them, masks [M, columns] shared by
    all classes, det_index {class: the columns of its detections, or None}.  -> ({class: sweep_class's dictionary}, mean AP float64 [M]:
    per configuration the mean over the classes, as `evaluate` forms it)."""
    if test_on not in CLASS_NAMES:
        raise ValueError("test_on is 'A', 'B' or 'AB'")
    rt = _runtime(rt)
    if gt_all is None:
        gt_all = benchmark_groundtruth(dataset_dir, idx_list)
    if not torch.is_tensor(masks):
        masks = torch.from_numpy(np.ascontiguousarray(np.asarray(masks) != 0, np.uint8)).to(rt.device)
    out = {}
    for name in CLASS_NAMES[test_on]:
        if name not in predictions:
            raise KeyError('no predictions for class %s' % name)
        out[name] = sweep_class(name, predictions[name], gt_all, masks, det_index.get(name), threshold, rt)
    ap = np.ascontiguousarray(np.stack([out[c]['ap'] for c in CLASS_NAMES[test_on]], 1))      # [M, classes]: a row's mean is np.mean of its list
    return out, np.mean(ap, axis=1)


def _columns(images, idx_list, what):
    """The position in idx_list of every image id (the first, should an id occur twice); ValueError for an id that is not in the list."""
    idx = np.asarray(idx_list, np.int64).reshape(-1)
    images = np.asarray(images, np.int64).reshape(-1)
    if len(images) == 0:
        return np.zeros(0, np.int32)
    if len(idx) == 0:
        raise ValueError('%s of image %d, and the image list is empty' % (what, images[0]))
    by = np.argsort(idx, kind='stable')
    k = np.minimum(np.searchsorted(idx[by], images), len(idx) - 1)
    bad = idx[by][k] != images
    if bad.any():
        raise ValueError('%s of image %d, which is not in the image list: its weight is not defined' % (what, images[bad][0]))
    return by[k].astype(np.int32)


def bootstrap_class(classname, det, gt, weights, idx_list, threshold=0.25, rt=None):
    """compute_pr_curve_3d(classname, det, gt) -- the point evaluation, its dictionary -- and the AP of the class on every redraw of the
    image list `idx_list` that `weights` (bootstrap.Weights over len(idx_list) columns) holds, in one t3d_sunrgbd_eval_bootstrap call
    (csrc/sunrgbd_bootstrap.hip): the matching is that of the point evaluation, only the weighted curve is formed per replicate.
    Column c of the weights is the image idx_list[c]; a detection or box of an image that is not in the list raises ValueError.
    -> the dictionary plus 'ap' float64 [R] and 'n_pos', 'n_tp', 'n_fp' int64 [R]."""
    rt = _runtime(rt)
    if weights.n_images != len(idx_list):
        raise ValueError('%d weight columns for %d images' % (weights.n_images, len(idx_list)))
    same = np.array([c == classname for c in gt['classname']], bool) if 'classname' in gt else np.ones(len(gt['image']), bool)
    own = select_boxes(gt, same)
    cols = (weights, _columns(det['image'], idx_list, 'a detection'), _columns(own['image'], idx_list, 'a ground-truth box'))
    launch, fetch = _eval_prepare(det, own, None, threshold, rt, boot=cols)
    launch()
    r = fetch()
    out = _pr_curve_result(r, same)
    out.update(r['boot'])
    return out


GT_STATES = ('claimed', 'localised', 'missed')              # gt_state 1, 2, 3 of t3d_sunrgbd_diagnose


def loc_summary(kind, loc_error):
    """The host's summary of loc_error [P,6], separately over the true positives and over the LOC detections: {'tp' | 'loc': {'n',
    and per abi.LOC_ERRORS column the median of its finite values (NaN when there is none: n == 0, or a box without volume)}}."""
    out = {}
    for group in ('tp', 'loc'):
        rows = np.asarray(loc_error, np.float64).reshape(-1, len(abi.LOC_ERRORS))[np.asarray(kind) == abi.DIAG_KINDS.index(group)]
        s = {'n': int(len(rows))}
        for k, name in enumerate(abi.LOC_ERRORS):
            v = rows[:, k][np.isfinite(rows[:, k])]
            s[name] = float(np.median(v)) if len(v) else float('nan')
        out[group] = s
    return out


def diagnose_class(classname, det, gt_all, threshold=0.25, bg_threshold=0.1, rt=None, classes=None, parts=False):
    """compute_pr_curve_3d(classname, det, gt_all) and the diagnosis of its errors (t3d_sunrgbd_diagnose, include/t3d.h), one call.
    gt_all holds the ground truth of every class ('classname' per box); classes: the evaluated set (default: every class of gt_all) --
    the boxes of its other members are what a detection can be confused with.  -> compute_pr_curve_3d's dictionary plus, in file
    order, kind (abi.DIAG_KINDS), otherOverlap, otherGt (1-based into gt_all, 0 = none); gtState over gt_all (1 claimed, 2 missed but
    localised, 3 missed; 0 for the boxes of other classes); counts {tp cls loc both dup bkg}, gtCounts {claimed localised missed},
    apFixed and dAP = apFixed - apScore {cls loc both dup bkg missed fp fn}.
    parts: one t3d_sunrgbd_locparts call in place of the diagnose call -- which parameter group makes a LOC detection loose.  The
    dictionary gains, in file order, partOverlap [P,5] (the overlap with its box once the detection's xy / z / centre / size / heading is
    the box's: abi.LOC_PARTS) and locError [P,6] (abi.LOC_ERRORS: centre distance in xy, dz, log size ratios l w h, heading in
    radians); partCounts (LOC detections each part repairs), partBoxes (boxes that gain a true positive), apPart and dAPPart = apPart -
    apScore, keyed by abi.LOC_PARTS; locSummary (`loc_summary`).  The parts do not add up: a detection may be repaired by several."""
    names = gt_all['classname']
    same = np.array([c == classname for c in names], bool)
    others = np.array([c != classname and (classes is None or c in classes) for c in names], bool)
    osel = np.nonzero(others)[0]
    r = _eval_call(det, select_boxes(gt_all, same), None, threshold, rt, other=select_boxes(gt_all, others), bg_threshold=bg_threshold,
                   parts=parts)
    out = _pr_curve_result(r, same)
    og = r['other_gt'].astype(np.int64)
    og[og > 0] = osel[og[og > 0] - 1] + 1
    state = np.zeros(len(names), np.uint8)
    state[same] = r['gt_state']
    ap_fixed = {k: float(v) for k, v in zip(abi.DIAG_FIXES, r['ap_fixed'])}
    out.update(kind=r['kind'], otherOverlap=r['other_overlap'], otherGt=og, gtState=state,
               counts={k: int(v) for k, v in zip(abi.DIAG_KINDS, r['counts'])}, gtCounts={k: int(v) for k, v in zip(GT_STATES, r['gt_counts'])},
               apFixed=ap_fixed, dAP={k: v - out['apScore'] for k, v in ap_fixed.items()})
    if parts:
        ap_part = {k: float(v) for k, v in zip(abi.LOC_PARTS, r['ap_part'])}
        loc_error = r['loc_error'].reshape(-1, len(abi.LOC_ERRORS))
        out.update(partOverlap=r['part_overlap'].reshape(-1, len(abi.LOC_PARTS)), locError=loc_error,
                   partCounts={k: int(v) for k, v in zip(abi.LOC_PARTS, r['part_counts'])},
                   partBoxes={k: int(v) for k, v in zip(abi.LOC_PARTS, r['part_boxes'])}, apPart=ap_part,
                   dAPPart={k: v - out['apScore'] for k, v in ap_part.items()}, locSummary=loc_summary(r['kind'], loc_error))
    return out


def _dap_text(dap):
    v = ['%s %.2f' % (k, 100.0 * dap[k]) for k in abi.DIAG_FIXES]
    return ' '.join(v[:6]) + ' | ' + ' '.join(v[6:])


def _loc_text(s):
    """`loc n 5 | xy 0.41 z +0.02 | l +35% w -3% h +1% | heading 12.0 deg` of one group of loc_summary; `-` for a value there is none of."""
    val = lambda k, fmt, f=lambda v: v: fmt % f(s[k]) if math.isfinite(s[k]) else '-'
    pct = lambda v: 100.0 * (math.exp(v) - 1.0)
    return 'loc n %d | xy %s z %s | l %s w %s h %s | heading %s deg' % (
        s['n'], val('xy', '%.2f'), val('z', '%+.2f'), val('l', '%+.0f%%', pct), val('w', '%+.0f%%', pct), val('h', '%+.0f%%', pct),
        val('heading', '%.1f', math.degrees))


def _dap_parts_text(dap):
    return ' '.join('%s %.2f' % (k, 100.0 * dap[k]) for k in abi.LOC_PARTS)


def bb3d_overlap_close_form(bb1, bb2, rt=None):
    """bb3dOverlapCloseForm.m: the dense [len(bb1), len(bb2)] score matrix of two box lists (every box on one pseudo-image)."""
    P, G = len(bb1['coeffs']), len(bb2['coeffs'])
    if P == 0 or G == 0:
        return np.zeros((0, 0))                                              # scoreMatrix = []  (bb3dOverlapCloseForm.m:6-9)
    det = dict(bb1, confidence=np.zeros(P), image=np.zeros(P, np.int32))
    gt = {k: bb2[k] for k in ('centroid', 'basis', 'coeffs')}
    gt['image'] = np.zeros(G, np.int32)
    r = _eval_call(det, gt, None, 0.25, rt, want_overlaps=True)
    m = np.zeros((P, G))
    m[np.repeat(np.arange(P), G), r['overlap_gt']] = r['overlaps']
    return m


def num2str(x):
    """MATLAB's num2str of a real scalar: an integer as %d, otherwise max(floor(log10(|x|)) + 5, 5) significant digits (at most 16)."""
    x = float(x)
    if math.isnan(x):
        return 'NaN'
    if math.isinf(x):
        return 'Inf' if x > 0 else '-Inf'
    if x == round(x):
        return '%d' % int(round(x))
    digits = min(max(int(math.floor(math.log10(abs(x)))) + 5, 5), 16)
    return ('%.*g' % (digits, x)).strip()


def evaluate(pred_dir, dataset_dir, idx_list, test_on='B', rt=None, log=print, threshold=0.25, save_curves=None, predictions=None,
             diagnose=None, bootstrap=None):
    """script_3Deval.m:33-60: per class of the set `test_on`, the number of predictions, the AP, and the mean AP, logged as the script
    displays them.  `predictions` ({class: boxes}, e.g. official_predictions of a test_semisup run) stands in for the files of `pred_dir`.
    -> ({class: AP}, mean AP).  save_curves: a directory for <class>_pr.npz.
    diagnose: None, or {'bg': the background overlap t_b (0.1), 'json': a path or None}: diagnose_class per class -- two more lines
    behind each AP line (the detections per kind and the boxes per state; 100 x dAP per fix), one behind the mean (the class means),
    the summary as JSON at the path, and the per-detection arrays in <class>_pr.npz.  With 'parts': True (diagnose_class(parts=True))
    two more lines behind each `dAP for` line -- `Localisation for X:` (the medians of the six errors over the LOC detections, sizes
    as 100 (exp(median log ratio) - 1) per cent) and `dAP(loc) for X:` (100 x dAPPart per part, beside the loc fix, and the detections
    each part repairs) -- and `Mean dAP(loc):` behind `Mean dAP:`; the JSON gains `parts` and `locSummary` per class, `loc_parts` and
    `mean_dAP_parts`; the .npz gains partOverlap and locError.
    bootstrap: None, the number of replicates, or {'R', 'seed' (0), 'level' (0.95), 'json' (a path or None), 'weights' (a
    bootstrap.Weights over the image list, made here when absent)}: bootstrap_class per class -- an `AP interval` line behind each AP
    line and a `Mean AP interval` line behind the mean (the percentile interval over R redraws of the image list, bootstrap.py) -- and
    the return value gains a third entry, {'R', 'seed', 'level', 'ap': {class: replicate APs [R]}, 'summary': bootstrap.summary}."""
    if test_on not in CLASS_NAMES:
        raise ValueError("test_on is 'A', 'B' or 'AB'")
    rt = _runtime(rt)
    if bootstrap is not None:
        from . import bootstrap as BS
        if diagnose is not None:
            raise ValueError('a diagnosis of the replicates is not defined: diagnose and bootstrap exclude each other')
        bootstrap = dict(bootstrap) if isinstance(bootstrap, dict) else {'R': int(bootstrap)}
        if isinstance(idx_list, str):
            idx_list = [int(line.rstrip()) for line in open(idx_list) if line.strip()]
        idx_list = list(idx_list)
        weights = bootstrap.get('weights') or BS.Weights(rt, len(idx_list), bootstrap['R'], bootstrap.get('seed', 0))
        level, boot_ap = bootstrap.get('level', 0.95), {}
    gt_all = benchmark_groundtruth(dataset_dir, idx_list)
    ap, summary = {}, {}
    parts = bool(diagnose is not None and diagnose.get('parts'))
    if save_curves:
        os.makedirs(save_curves, exist_ok=True)
    for name in CLASS_NAMES[test_on]:
        if predictions is not None:
            if name not in predictions:
                raise KeyError('no predictions for class %s' % name)
            det = predictions[name]
        else:
            det = parse_class_predictions(os.path.join(pred_dir, name + '_pred.txt'), name)
        log('Number of predictions for %s: %d' % (name.upper(), len(det['confidence'])))
        if bootstrap is not None:
            r = bootstrap_class(name, det, gt_all, weights, idx_list, threshold, rt)
        elif diagnose is None:
            r = compute_pr_curve_3d(name, det, gt_all, None, threshold, rt)
        else:
            r = diagnose_class(name, det, gt_all, threshold, diagnose.get('bg', 0.1), rt, classes=CLASS_NAMES[test_on], parts=parts)
        log('AP Score for %s: [%s]' % (name.upper(), num2str(r['apScore'] * 100.0)))
        ap[name] = r['apScore']
        if bootstrap is not None:
            boot_ap[name] = r['ap']
            log('AP interval for %s: %s' % (name.upper(), BS.interval_text(BS.summary({name: r['ap']}, level)['classes'][name], level, weights.R, num2str)))
        curves = dict(precision=r['precision'], recall=r['recall'], isTp=r['isTp'], isFp=r['isFp'], maxOverlaps=r['maxOverlaps'],
                      gtAssignment=r['gtAssignment'], isMissed=r['isMissed'])
        if diagnose is not None:
            c, g = r['counts'], r['gtCounts']
            log('Diagnosis for %s: %s | boxes %d missed %d localised %d' % (name.upper(), ' '.join('%s %d' % (k, c[k]) for k in abi.DIAG_KINDS),
                                                                           r['numOfgt'], g['missed'], g['localised']))
            log('dAP for %s: %s' % (name.upper(), _dap_text(r['dAP'])))
            summary[name] = {'ap': r['apScore'], 'predictions': len(det['confidence']), 'boxes': r['numOfgt'], 'counts': c, 'gtCounts': g,
                             'apFixed': r['apFixed'], 'dAP': r['dAP']}
            curves.update(kind=r['kind'], otherOverlap=r['otherOverlap'], otherGt=r['otherGt'], gtState=r['gtState'])
            if parts:
                log('Localisation for %s: %s' % (name.upper(), _loc_text(r['locSummary']['loc'])))
                log('dAP(loc) for %s: %s | of loc %.2f | repaired %s of %d' % (name.upper(), _dap_parts_text(r['dAPPart']), 100.0 * r['dAP']['loc'],
                                                                             ' '.join('%d' % r['partCounts'][k] for k in abi.LOC_PARTS), c['loc']))
                summary[name].update(parts={'apPart': r['apPart'], 'dAPPart': r['dAPPart'], 'partCounts': r['partCounts'], 'partBoxes': r['partBoxes']},
                                     locSummary=r['locSummary'])
                curves.update(partOverlap=r['partOverlap'], locError=r['locError'])
        if save_curves:
            np.savez(os.path.join(save_curves, name + '_pr.npz'), **curves)
    mean_ap = float(np.mean([ap[c] for c in CLASS_NAMES[test_on]]))
    log('Mean AP Score: [%s]' % num2str(mean_ap * 100.0))
    if diagnose is not None:
        mean_dap = {k: float(np.mean([summary[c]['dAP'][k] for c in CLASS_NAMES[test_on]])) for k in abi.DIAG_FIXES}
        log('Mean dAP: %s' % _dap_text(mean_dap))
        doc = {'test_on': test_on, 'threshold': threshold, 'bg_threshold': diagnose.get('bg', 0.1), 'kinds': list(abi.DIAG_KINDS),
               'fixes': list(abi.DIAG_FIXES), 'classes': summary, 'mean_ap': mean_ap, 'mean_dAP': mean_dap}
        if parts:
            mean_parts = {k: float(np.mean([summary[c]['parts']['dAPPart'][k] for c in CLASS_NAMES[test_on]])) for k in abi.LOC_PARTS}
            log('Mean dAP(loc): %s' % _dap_parts_text(mean_parts))
            doc.update(loc_parts=list(abi.LOC_PARTS), mean_dAP_parts=mean_parts)
        if diagnose.get('json'):
            with open(diagnose['json'], 'w') as fh:
                json.dump(doc, fh, indent=1)
    if bootstrap is not None:
        boot = {'R': weights.R, 'seed': weights.seed, 'level': level, 'ap': boot_ap, 'summary': BS.summary(boot_ap, level)}
        log('Mean AP interval: %s' % BS.interval_text(boot['summary']['mean_ap'], level, weights.R, num2str))
        if bootstrap.get('json'):
            with open(bootstrap['json'], 'w') as fh:
                json.dump(bootstrap_json(test_on, threshold, ap, mean_ap, boot), fh, indent=1)
        return ap, mean_ap, boot
    return ap, mean_ap


def bootstrap_json(test_on, threshold, ap, mean_ap, boot):
    """What --bootstrap_json holds for one evaluation: the point APs, every class's replicate APs and the summaries."""
    return {'test_on': test_on, 'threshold': threshold, 'R': boot['R'], 'seed': boot['seed'], 'level': boot['level'],
            'ap': {c: float(v) for c, v in ap.items()}, 'mean_ap': mean_ap, 'replicates': {c: [float(x) for x in v] for c, v in boot['ap'].items()},
            'summary': boot['summary']}


def compare(pred_dir_a, pred_dir_b, dataset_dir, idx_list, test_on='B', rt=None, log=print, threshold=0.25, bootstrap=None):
    """`evaluate` on two prediction directories against the same ground truth with the SAME bootstrap weights -- the paired bootstrap,
    each image its own control -- e.g. a run with and one without --nms_fuse.  Both sets of lines are logged, tagged `A: ` and `B: `,
    then per class and for the mean `dAP for X (B - A): mean [lo, hi], p(≤0) share` (x 100; bootstrap.paired).
    -> (evaluate's triple for A, for B, bootstrap.paired of the two)."""
    from . import bootstrap as BS
    if bootstrap is None:
        raise ValueError('a comparison needs the bootstrap')
    rt = _runtime(rt)
    bootstrap = dict(bootstrap) if isinstance(bootstrap, dict) else {'R': int(bootstrap)}
    if isinstance(idx_list, str):
        idx_list = [int(line.rstrip()) for line in open(idx_list) if line.strip()]
    idx_list = list(idx_list)
    shared = dict(bootstrap, json=None, weights=bootstrap.get('weights') or BS.Weights(rt, len(idx_list), bootstrap['R'], bootstrap.get('seed', 0)))
    a = evaluate(pred_dir_a, dataset_dir, idx_list, test_on, rt=rt, log=lambda t: log('A: ' + t), threshold=threshold, bootstrap=shared)
    b = evaluate(pred_dir_b, dataset_dir, idx_list, test_on, rt=rt, log=lambda t: log('B: ' + t), threshold=threshold, bootstrap=shared)
    d = BS.paired(a[2]['ap'], b[2]['ap'], a[2]['level'])
    for name in CLASS_NAMES[test_on]:
        log('dAP for %s (B - A): %s' % (name.upper(), BS.difference_text(d['classes'][name])))
    log('Mean dAP (B - A): %s' % BS.difference_text(d['mean_ap']))
    if bootstrap.get('json'):
        with open(bootstrap['json'], 'w') as fh:
            json.dump({'A': bootstrap_json(test_on, threshold, a[0], a[1], a[2]), 'B': bootstrap_json(test_on, threshold, b[0], b[1], b[2]),
                       'paired': d}, fh, indent=1)
    return a, b, d


def official_predictions(test_classes, predictions, class_names):
    """The boxes parse_class_predictions would read from the files test_semisup.write_detection_results writes, from test_semisup's
    14-list held in memory (from_prediction_to_label_format per detection, no text round trip): {class: boxes} for `evaluate`."""
    from .test_semisup import from_prediction_to_label_format
    _, _, _, center_l, hcls_l, hres_l, scls_l, sres_l, rot_l, score_l, _, id_l, _, _ = predictions
    rows = {c: [] for c in test_classes}
    decoded = getattr(predictions, 'decoded', None)          # semisup_infer --device_decode: the label rows of t3d_detect_decode
    for i in range(len(center_l)):
        if decoded is not None:
            vals = decoded.label[i]
        else:
            vals = from_prediction_to_label_format(center_l[i], hcls_l[i], hres_l[i], scls_l[i], sres_l[i], float(rot_l[i]))
        rows[class_names[i]].append((int(id_l[i]),) + tuple(float(v) for v in vals) + (float(score_l[i]),))
    out = {}
    for c, r in rows.items():
        a = np.asarray(r, np.float64).reshape(-1, 9)
        out[c] = boxes_from_label_format(a[:, 0].astype(np.int64), *[a[:, k] for k in range(1, 9)])
    return out


def official_eval_of_test_semisup(test_semisup_argv, dataset_dir, idx_list, test_on='AB', rt=None, log=print, threshold=0.25, save_curves=None,
                                  diagnose=None, bootstrap=None):
    """test_semisup's run (its own command line: a frustum file with --data_path, or its synthetic frustums, whose image ids are their
    indices), then `evaluate` on the predictions it returns.  With --result_dir among its flags the same run also writes the
    <class>_pred.txt files."""
    from . import semisup_infer as TS              # test_semisup's driver, plus --device_decode
    from .constants import class2type
    FLAGS = TS.build_flags(list(test_semisup_argv))
    predictions = TS.test(FLAGS, rt=rt, log=log)
    names = [class2type[int(c)] for c in predictions[10]]
    held = official_predictions(sorted(set(CLASS_NAMES[test_on]) | set(names)), predictions, names)
    if rt is None:
        rt = _runtime(None)
    return evaluate(None, dataset_dir, idx_list, test_on, rt=rt, log=log, threshold=threshold, save_curves=save_curves, predictions=held,
                    diagnose=diagnose, bootstrap=bootstrap)


def add_diagnose_arguments(p):
    """--diagnose and its three options, for this parser and for detect's."""
    p.add_argument('--diagnose', action='store_true',
                   help='sort the errors of every class into kinds and print what fixing each kind would add to its AP (module docstring)')
    p.add_argument('--diagnose_bg', type=float, default=None, help='--diagnose: the overlap below which a detection is on nothing (default 0.1)')
    p.add_argument('--diagnose_json', default=None, help='--diagnose: write the summary (counts, AP per fix, dAP, means) to this file')
    p.add_argument('--diagnose_parts', action='store_true',
                   help='--diagnose: split the localisation errors into xy, z, centre, size and heading -- what each costs and repairs')


def diagnose_options(p, FLAGS, threshold=0.25):
    """The `diagnose` dictionary of `evaluate` from parsed flags (None without --diagnose); a parser error where they contradict."""
    if not FLAGS.diagnose:
        if FLAGS.diagnose_bg is not None or FLAGS.diagnose_json is not None or FLAGS.diagnose_parts:
            p.error('--diagnose_bg / --diagnose_json / --diagnose_parts need --diagnose')
        return None
    bg = 0.1 if FLAGS.diagnose_bg is None else FLAGS.diagnose_bg
    if not 0.0 <= bg < threshold:
        p.error('--diagnose_bg must lie in [0, %g), below the overlap a true positive needs' % threshold)
    return {'bg': bg, 'json': FLAGS.diagnose_json, 'parts': bool(FLAGS.diagnose_parts)}


def parser():
    p = argparse.ArgumentParser(description='SUN-RGBD 3-D detection AP by the protocol of script_3Deval.m, on the device',
                                allow_abbrev=False)      # (--test is test_semisup's flag, not a short form of --test_on)
    p.add_argument('--pred_dir', default=None, help='directory of <class>_pred.txt files (test_semisup --result_dir)')
    p.add_argument('--official_eval', action='store_true',
                   help='run test_semisup (every flag this parser does not know is passed to it) and score the predictions it holds in memory')
    p.add_argument('--dataset_dir', default='mysunrgbd', help='SUN-RGBD root (<dir>/training/label_dimension)')
    p.add_argument('--idx_path', required=True, help='index file of the test images, e.g. mysunrgbd/training/val_data_idx.txt')
    p.add_argument('--test_on', default='B', choices=['A', 'B', 'AB'], help='set of classes to test on')
    p.add_argument('--threshold', type=float, default=0.25, help='overlap a true positive needs (the script: 0.25)')
    p.add_argument('--save_curves', default=None, help='directory for <class>_pr.npz (precision, recall, isTp, isFp, ...)')
    p.add_argument('--gpu', type=int, default=0)
    add_diagnose_arguments(p)
    from . import bootstrap as BS
    BS.add_arguments(p)
    p.add_argument('--compare_pred_dir', default=None,
                   help='--pred_dir A --compare_pred_dir B --bootstrap R: both directories against the same ground truth with the same redraws, '
                        'and the paired interval of B - A per class and for the mean')
    return p


def main(argv=None, rt=None, log=print):
    FLAGS, rest = parser().parse_known_args(argv)
    diagnose = diagnose_options(parser(), FLAGS, FLAGS.threshold)
    from . import bootstrap as BS
    bootstrap = BS.options(parser(), FLAGS)
    if FLAGS.compare_pred_dir is not None and (bootstrap is None or FLAGS.official_eval or not FLAGS.pred_dir or FLAGS.save_curves):
        parser().error('--compare_pred_dir needs --pred_dir and --bootstrap (and takes neither --official_eval nor --save_curves)')
    if rt is None and torch.cuda.is_available():
        torch.cuda.set_device(FLAGS.gpu)
    if FLAGS.official_eval:
        rest = list(rest) + ['--gpu', str(FLAGS.gpu)]                     # the one flag both parsers have: test_semisup gets it too
        return official_eval_of_test_semisup(rest, FLAGS.dataset_dir, FLAGS.idx_path, FLAGS.test_on, rt=rt, log=log, threshold=FLAGS.threshold,
                                             save_curves=FLAGS.save_curves, diagnose=diagnose, bootstrap=bootstrap)
    if rest or not FLAGS.pred_dir:
        parser().error('--pred_dir is required' if not rest else 'unrecognized arguments: %s' % ' '.join(rest))
    if FLAGS.compare_pred_dir is not None:
        return compare(FLAGS.pred_dir, FLAGS.compare_pred_dir, FLAGS.dataset_dir, FLAGS.idx_path, FLAGS.test_on, rt=rt, log=log,
                       threshold=FLAGS.threshold, bootstrap=bootstrap)
    return evaluate(FLAGS.pred_dir, FLAGS.dataset_dir, FLAGS.idx_path, FLAGS.test_on, rt=rt, log=log, threshold=FLAGS.threshold,
                    save_curves=FLAGS.save_curves, diagnose=diagnose, bootstrap=bootstrap)


if __name__ == '__main__':
    main()
