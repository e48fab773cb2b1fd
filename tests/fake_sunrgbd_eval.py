"""TEST INFRASTRUCTURE ONLY -- NumPy executable specification of t3d_sunrgbd_eval (include/t3d.h, csrc/sunrgbd_eval.hip), on host
pointers, so that transferable3d_amd/evaluate_sunrgbd.py and its command line run end to end through
Runtime(device='cpu', lib=FakeSunrgbdEvalLib()).  The stages are the entry point's (rank by counting, per-image ground truth, minimum
sorted position per box, integer scans); the box geometry is tests/ref_sunrgbd_eval.py's."""
import numpy as np

import ref_sunrgbd_eval as R
from fake_t3d import AbiSizeError, FakeLib, _struct, arr
from transferable3d_amd import abi

UNCLAIMED = 0x7fffffff


class FakeSunrgbdEvalLib(FakeLib):
    def t3d_sunrgbd_eval(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if not p.ap:
            return -1
        P, G, NI = p.P, p.G, p.n_images
        if P < 0 or G < 0 or NI < 0:
            return -2
        if P + G > 0 and (not p.workspace or p.workspace_bytes < abi.sunrgbd_eval_workspace_bytes(P, G)):
            return -1
        box = lambda c, b, k, n: [R.to_vector({'centroid': arr(c, n, 3)[i], 'basis': arr(b, n, 3, 3)[i], 'coeffs': arr(k, n, 3)[i]}) for i in range(n)]
        fd, fg = box(p.det_centroid, p.det_basis, p.det_coeffs, P), box(p.gt_centroid, p.gt_basis, p.gt_coeffs, G)
        conf, dimg, gimg = arr(p.det_confidence, P), arr(p.det_image, P), arr(p.gt_image, G)
        diff = arr(p.gt_difficult, G) if G and p.gt_difficult else np.zeros(G, np.uint8)
        ids, off, lst = arr(p.image_ids, NI), arr(p.image_gt_offsets, NI + 1), arr(p.image_gt, G)
        rank = np.zeros(P, np.int64)
        for i in range(P):                      # rank_i = #{s_j > s_i} + #{j < i : s_j = s_i}
            rank[i] = np.sum(conf > conf[i]) + np.sum(conf[:i] == conf[i])
        order = arr(p.order, P)
        if P:
            order[rank] = np.arange(P)
        first = np.full(G, UNCLAIMED, np.int64)
        mo, gi = arr(p.max_overlap, P), arr(p.gt_idx, P)
        ovo = arr(p.overlap_offsets, P + 1) if p.overlaps else None
        for i in range(P):
            k = int(np.searchsorted(ids, dimg[i])) if NI else 0
            g0, g1 = (int(off[k]), int(off[k + 1])) if k < NI and ids[k] == dimg[i] else (0, 0)
            best, best_g = 0.0, -1
            for n, q in enumerate(range(g0, g1)):
                g = int(lst[q])
                ov = R.overlap(fd[i], fg[g]) if gimg[g] == dimg[i] else 0.0
                if ov > best:
                    best, best_g = ov, g
                if ovo is not None and ovo[i] + n < ovo[i + 1]:
                    arr(p.overlaps, int(ovo[P]))[ovo[i] + n] = ov
                    arr(p.overlap_gt, int(ovo[P]))[ovo[i] + n] = g
            if best < R.EPS:
                best_g = -1
            mo[i], gi[i] = best, best_g + 1
            if best_g >= 0 and best >= p.threshold:
                first[best_g] = min(first[best_g], rank[i])
        tp, fp, ga = arr(p.is_tp, P), arr(p.is_fp, P), arr(p.gt_assignment, P)
        for i in range(P):
            g = int(gi[i]) - 1
            claims = g >= 0 and mo[i] >= p.threshold
            is_first = claims and first[g] == rank[i]
            dc = claims and diff[g] != 0
            tp[i], fp[i], ga[i] = int(is_first and not dc), int(not is_first and not dc), g + 1 if is_first else 0
        if G:
            arr(p.is_missed, G)[:] = first == UNCLAIMED
        n_pos = int(np.sum(diff == 0))
        ap = 0.0
        if P:
            ctp, cfp = np.cumsum(tp[order].astype(np.int64)), np.cumsum(fp[order].astype(np.int64))
            with np.errstate(invalid='ignore', divide='ignore'):
                rec = ctp.astype(np.float64) / np.float64(n_pos) if G else np.zeros(P)
                pre = ctp.astype(np.float64) / (cfp.astype(np.float64) + ctp.astype(np.float64))
            arr(p.recall, P)[:], arr(p.precision, P)[:] = rec, pre
            ap = R.get_average_precision(pre, rec)
        arr(p.ap, 1)[0] = ap
        return 0
