"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_sunrgbd_locparts (include/t3d.h, csrc/sunrgbd_locparts.hip) on
host pointers, so that evaluate_sunrgbd.diagnose_class(parts=True) and both command lines run end to end through
Runtime(device='cpu', lib=FakeSunrgbdLocPartsLib()).  The stages are the entry point's: the diagnosis (FakeSunrgbdDiagnoseLib), the rows
and their pairing, the six errors, the five counterfactual boxes and their overlaps with the matched box, the minimum sorted position of
a repaired detection per box and part, the counts and the five curves; the box geometry is tests/ref_sunrgbd_eval.py's and the AP
function fake_sunrgbd_diagnose.curve_ap."""
import numpy as np

import ref_sunrgbd_eval as R
from fake_sunrgbd_diagnose import LOC, TP, FakeSunrgbdDiagnoseLib, curve_ap
from fake_sunrgbd_eval import UNCLAIMED
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

XY, Z, CENTRE, SIZE, HEADING = range(5)


def rows_of(basis):
    """(vertical row, the two horizontal rows in row order): the vertical one has the largest |z component|, the first on ties."""
    v = int(np.argmax(np.abs(np.asarray(basis)[:, 2])))
    h = [r for r in range(3) if r != v]
    return v, h[0], h[1]


def pairing(A, B):
    """-> (p, q, partner: row of A -> row of B)."""
    va, a0, a1 = rows_of(A['basis'])
    vb, b0, b1 = rows_of(B['basis'])
    dot = lambda r, s: abs(A['basis'][r][0] * B['basis'][s][0] + A['basis'][r][1] * B['basis'][s][1])
    p, q = dot(a0, b0), dot(a0, b1)
    return p, q, ({va: vb, a0: b0, a1: b1} if p >= q else {va: vb, a0: b1, a1: b0})


def loc_errors(A, B):
    p, q, to_b = pairing(A, B)
    to_a = {s: r for r, s in to_b.items()}
    vb, b0, b1 = rows_of(B['basis'])
    sa, sb = np.abs(np.asarray(A['coeffs'], np.float64)), np.abs(np.asarray(B['coeffs'], np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        size = [np.log(sa[to_a[s]] / sb[s]) for s in (b0, b1, vb)]
    return [np.hypot(A['centroid'][0] - B['centroid'][0], A['centroid'][1] - B['centroid'][1]), A['centroid'][2] - B['centroid'][2]] + size + \
        [np.arctan2(min(p, q), max(p, q))]


def counterfactual(A, B, part):
    """The detection A with one parameter group taken from its box B; the rows stay in the order of the box they come from."""
    ce, basis, co = np.array(A['centroid'], np.float64), np.array(A['basis'], np.float64), np.array(A['coeffs'], np.float64)
    bc = np.asarray(B['centroid'], np.float64)
    if part in (XY, CENTRE):
        ce[:2] = bc[:2]
    if part in (Z, CENTRE):
        ce[2] = bc[2]
    if part in (SIZE, HEADING):
        _, _, to_b = pairing(A, B)
        sa, sb = np.abs(np.asarray(A['coeffs'], np.float64)), np.abs(np.asarray(B['coeffs'], np.float64))
        if part == SIZE:
            co = np.array([sb[to_b[r]] for r in range(3)])
        else:
            to_a = {s: r for r, s in to_b.items()}
            basis, co = np.array(B['basis'], np.float64), np.array([sa[to_a[s]] for s in range(3)])
    return {'centroid': ce, 'basis': basis, 'coeffs': co}


def footprint(box):
    """The 10-vector of a box, and whether it has volume (a box without overlaps nothing)."""
    v = R.to_vector(box)
    return v, R.cuboid_volume(v) > 0


_PAIR_MEMO = {}      # (bytes of A, bytes of B) -> (|p - q|, the six errors, the five overlaps): a second call on the same boxes clips nothing


def measure(A, B):
    key = tuple(np.ascontiguousarray(x[k], np.float64).tobytes() for x in (A, B) for k in ('centroid', 'basis', 'coeffs'))
    if key not in _PAIR_MEMO:
        pp, qq, _ = pairing(A, B)
        fb, solid_b = footprint(B)
        ov = []
        for f in range(5):
            fa, solid_a = footprint(counterfactual(A, B, f))
            ov.append(R.overlap(fa, fb) if solid_a and solid_b else 0.0)
        _PAIR_MEMO[key] = (abs(pp - qq), loc_errors(A, B), ov)
    return _PAIR_MEMO[key]


class FakeSunrgbdLocPartsLib(FakeSunrgbdDiagnoseLib):
    def t3d_sunrgbd_locparts(self, a, d, q_, stream):
        try:
            p, q, s = _struct(a), _struct(d), _struct(q_)
        except AbiSizeError:
            return abi.ERR_ABI
        if s.reserved != 0 or not s.part_counts or not s.part_boxes or not s.ap_part:
            return -1
        P, G = p.P, p.G
        if P > 0 and (not s.part_overlap or not s.loc_error):
            return -1
        if G > 0 and (not s.workspace or s.workspace_bytes < abi.sunrgbd_locparts_workspace_bytes(P, G)):
            return -1
        e = self.t3d_sunrgbd_diagnose(a, d, stream)
        if e != 0:
            return e
        t_f = p.threshold
        box = lambda c, b, k, n, i: {'centroid': arr(c, n, 3)[i], 'basis': arr(b, n, 3, 3)[i], 'coeffs': arr(k, n, 3)[i]}
        gi, kind, order = arr(p.gt_idx, P), arr(q.kind, P), arr(p.order, P)
        state = arr(q.gt_state, G) if G else np.zeros(0, np.uint8)
        rank = np.zeros(P, np.int64)
        if P:
            rank[order] = np.arange(P)
        ov = arr(s.part_overlap, P, 5) if P else np.zeros((0, 5))
        err = arr(s.loc_error, P, 6) if P else np.zeros((0, 6))
        first = np.full((5, G), UNCLAIMED, np.int64)
        self.last_pairing_gap = gaps = np.full(P, np.inf)                   # |p - q| per matched detection (for the tests)
        for i in range(P):
            g = int(gi[i]) - 1
            if g < 0:
                ov[i], err[i] = 0.0, np.nan
                continue
            A, B = box(p.det_centroid, p.det_basis, p.det_coeffs, P, i), box(p.gt_centroid, p.gt_basis, p.gt_coeffs, G, g)
            gaps[i], err[i], ov[i] = measure(A, B)
            for f in range(5):
                if kind[i] == LOC and ov[i, f] >= t_f:
                    first[f, g] = min(first[f, g], rank[i])
        kinds = np.array(kind[:P], np.int64) if P else np.zeros(0, np.int64)
        out = arr(s.ap_part, 5)
        for f in range(5):
            repaired = (kinds == LOC) & (ov[:, f] >= t_f) if P else np.zeros(0, bool)
            promoted = np.zeros(P, bool)
            for i in np.nonzero(repaired)[0]:
                g = int(gi[i]) - 1
                promoted[i] = g >= 0 and state[g] == 2 and first[f, g] == rank[i]
            arr(s.part_counts, 5)[f] = int(repaired.sum())
            arr(s.part_boxes, 5)[f] = int(np.sum((state == 2) & (first[f] != UNCLAIMED))) if G else 0
            t, fp = (kinds == TP) | promoted, (kinds != TP) & ~repaired
            out[f] = curve_ap(t[order], fp[order], G) if P else 0.0
        return 0
