"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_sunrgbd_diagnose (include/t3d.h, csrc/sunrgbd_diagnose.hip) on
host pointers, so that evaluate_sunrgbd.diagnose_class and both command lines run end to end through
Runtime(device='cpu', lib=FakeSunrgbdDiagnoseLib()).  The stages are the entry point's: the evaluation (FakeSunrgbdEvalLib), the overlaps
with the other-class boxes of the same image, the kinds, the minimum sorted position of a LOC detection per box, the states, the counts
and the eight curves; the box geometry and the AP function are tests/ref_sunrgbd_eval.py's."""
import numpy as np

import ref_sunrgbd_eval as R
from fake_sunrgbd_eval import UNCLAIMED, FakeSunrgbdEvalLib
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

TP, CLS, LOC, BOTH, DUP, BKG = range(6)
FIX_CLS, FIX_LOC, FIX_BOTH, FIX_DUP, FIX_BKG, FIX_MISSED, FIX_FP, FIX_FN = range(8)
REMOVED = {FIX_CLS: CLS, FIX_BOTH: BOTH, FIX_DUP: DUP, FIX_BKG: BKG}


def curve_ap(tp, fp, n_pos):
    """The AP of 0/1 arrays in sorted order (a detection with 0 and 0 counts in neither sum) over n_pos boxes; no box: 0."""
    if len(tp) == 0 or n_pos <= 0:
        return 0.0
    ctp, cfp = np.cumsum(tp.astype(np.int64)), np.cumsum(fp.astype(np.int64))
    with np.errstate(invalid='ignore', divide='ignore'):
        rec = ctp.astype(np.float64) / np.float64(n_pos)
        pre = ctp.astype(np.float64) / (cfp.astype(np.float64) + ctp.astype(np.float64))
    return R.get_average_precision(pre, rec)


class FakeSunrgbdDiagnoseLib(FakeSunrgbdEvalLib):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.other_memo = {}                          # (footprint bytes, footprint bytes) -> overlap: a second call on the same boxes clips nothing

    def _other_overlap(self, a, b):
        key = (a.tobytes(), b.tobytes())
        if key not in self.other_memo:
            self.other_memo[key] = R.overlap(a, b)
        return self.other_memo[key]

    def t3d_sunrgbd_diagnose(self, a, d, stream):
        try:
            p, q = _struct(a), _struct(d)
        except AbiSizeError:
            return abi.ERR_ABI
        if not q.counts or not q.gt_counts or not q.ap_fixed or p.gt_difficult:
            return -1
        if not (q.bg_threshold >= 0.0 and q.bg_threshold < p.threshold):
            return -1
        P, G, Go, NO = p.P, p.G, q.Go, q.n_other_images
        if P < 0 or G < 0 or Go < 0 or NO < 0:
            return -2
        if G + Go > 0 and (not q.workspace or q.workspace_bytes < abi.sunrgbd_diagnose_workspace_bytes(P, G, Go)):
            return -1
        e = self.t3d_sunrgbd_eval(a, stream)
        if e != 0:
            return e
        t_f, t_b = p.threshold, q.bg_threshold
        box = lambda c, b, k, n: [R.to_vector({'centroid': arr(c, n, 3)[i], 'basis': arr(b, n, 3, 3)[i], 'coeffs': arr(k, n, 3)[i]}) for i in range(n)]
        fd, fo = box(p.det_centroid, p.det_basis, p.det_coeffs, P), box(q.other_centroid, q.other_basis, q.other_coeffs, Go)
        dimg, oimg = arr(p.det_image, P), arr(q.other_image, Go)
        ids, off, lst = arr(q.other_image_ids, NO), arr(q.other_image_offsets, NO + 1), arr(q.other_image_list, Go)
        mo, gi, tp = arr(p.max_overlap, P), arr(p.gt_idx, P), arr(p.is_tp, P)
        order = arr(p.order, P)
        rank = np.zeros(P, np.int64)
        if P:
            rank[order] = np.arange(P)
        oo, og, kind = arr(q.other_overlap, P), arr(q.other_gt, P), arr(q.kind, P)
        loc_first = np.full(G, UNCLAIMED, np.int64)
        self.last_other_overlaps = rows = []          # per detection, every overlap with the other-class boxes of its image (for the tests)
        for i in range(P):
            k = int(np.searchsorted(ids, dimg[i])) if NO else 0
            g0, g1 = (int(off[k]), int(off[k + 1])) if k < NO and ids[k] == dimg[i] else (0, 0)
            best, best_g = 0.0, -1
            rows.append([])
            for n in range(g0, g1):
                g = int(lst[n])
                ov = self._other_overlap(fd[i], fo[g]) if oimg[g] == dimg[i] else 0.0
                rows[-1].append(ov)
                if ov > best:
                    best, best_g = ov, g
            if best < R.EPS:
                best_g = -1
            oo[i], og[i] = best, best_g + 1
            if tp[i]:
                kind[i] = TP
            elif mo[i] >= t_f:
                kind[i] = DUP
            elif mo[i] >= t_b:
                kind[i] = LOC
            elif best >= t_f:
                kind[i] = CLS
            elif best >= t_b:
                kind[i] = BOTH
            else:
                kind[i] = BKG
            if kind[i] == LOC and gi[i] > 0:
                loc_first[gi[i] - 1] = min(loc_first[gi[i] - 1], rank[i])
        state = np.zeros(G, np.uint8)
        if G:
            missed = arr(p.is_missed, G) != 0
            state[:] = np.where(~missed, 1, np.where(loc_first != UNCLAIMED, 2, 3))
            arr(q.gt_state, G)[:] = state
        kinds = np.array(kind[:P], np.int64) if P else np.zeros(0, np.int64)
        arr(q.counts, 6)[:] = [int(np.sum(kinds == k)) for k in range(6)]
        arr(q.gt_counts, 3)[:] = [int(np.sum(state == s)) for s in (1, 2, 3)]
        ks = kinds[order] if P else kinds                                    # sorted order
        promoted = np.zeros(P, bool)
        for i in range(P):
            g = int(gi[i]) - 1
            promoted[i] = kinds[i] == LOC and g >= 0 and state[g] == 2 and loc_first[g] == rank[i]
        out = arr(q.ap_fixed, 8)
        for fix in range(8):
            t, f, n_pos = ks == TP, ks != TP, G
            if fix in REMOVED:
                f = f & (ks != REMOVED[fix])
            elif fix == FIX_LOC:
                t, f = t | promoted[order], f & (ks != LOC)
            elif fix == FIX_MISSED:
                n_pos = G - int(np.sum(state == 3))
            elif fix == FIX_FP:
                f = np.zeros(P, bool)
            elif fix == FIX_FN:
                n_pos = G - int(np.sum(state >= 2))
            out[fix] = curve_ap(t, f, n_pos)
        return 0
