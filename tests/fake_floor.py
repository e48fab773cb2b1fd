"""TEST INFRASTRUCTURE ONLY -- NumPy executable specification of t3d_scene_floor and t3d_detect_floor (include/t3d.h, csrc/floor.hip), on
host pointers, so that transferable3d_amd/floor.py and the stages behind the decode run through Runtime(device='cpu', lib=FakeFloorLib()).
Every expression is the header's, elementwise fp64 in the stated order -- the order of the sums included: lane, halving tree, chunk,
workgroup."""
import numpy as np

from fake_scene import FakeSceneLib
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

CHUNK, BLOCKS, LANES = abi.SCENE_FLOOR_CHUNK, abi.SCENE_FLOOR_BLOCKS, 256
NAN_BITS = 0x7FF8000000000000
OPTIONS = dict(z_lo=-3.0, z_hi=-0.2, bin=0.02, inv_bin=1.0 / 0.02, n_bins=140, min_share=0.02, min_inliers=50, band=0.05,
               max_slope2=float(np.tan(np.radians(5.0)) ** 2), min_spread=0.25, min_det_ratio=0.05)


def ordered_sums(terms, inlier):
    """The header's sum of every column of terms [n, K] over the rows `inlier` [n] -> [K]."""
    n, K = terms.shape
    n_chunks = -(-n // CHUNK)
    if n_chunks == 0:
        return np.zeros(K)
    t = np.zeros((n_chunks * CHUNK, K))
    m = np.zeros(n_chunks * CHUNK, bool)
    t[:n], m[:n] = terms, inlier
    t, m = t.reshape(n_chunks, CHUNK // LANES, LANES, K), m.reshape(n_chunks, CHUNK // LANES, LANES, 1)
    v = np.zeros((n_chunks, LANES, K))
    for r in range(CHUNK // LANES):                      # lane t: its inliers t, t + 256, ... in ascending order
        v = np.where(m[:, r], v + t[:, r], v)
    s = LANES // 2
    while s >= 1:                                        # v[t] = v[t] + v[t+s] for t < s
        v = v[:, :s] + v[:, s:2 * s]
        s //= 2
    chunk = v[:, 0]                                      # [n_chunks, K]
    total = np.zeros(K)
    for j in range(BLOCKS):                              # workgroup j: its chunks j, j + BLOCKS, ... ascending, from 0.0
        w = np.zeros(K)
        for c in range(j, n_chunks, BLOCKS):
            w = w + chunk[c]
        total = total + w
    return total


def scene_floor(points, o=OPTIONS):
    """One scene's outputs: (plane [8], counts [4] int32, hist [n_bins] int32).  points [n, >= 3]."""
    nb = o['n_bins']
    plane, counts, hist = np.zeros(8), np.zeros(4, np.int32), np.zeros(nb, np.int32)
    x, y, z = (np.ascontiguousarray(points[:, k], np.float64) for k in range(3))
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    counts[0] = n_finite = int(fin.sum())
    with np.errstate(invalid='ignore', over='ignore'):
        t = (z - o['z_lo']) * o['inv_bin']
        binned = fin & (t >= 0.0) & (t < float(nb))
    hist += np.bincount(np.floor(t[binned]).astype(np.int64), minlength=nb).astype(np.int32)
    h = np.concatenate([[0, 0, 0], hist.astype(np.int64), [0, 0, 0]])
    c3 = h[:-2] + h[1:-1] + h[2:]                        # c3[b] at index b + 2, for b = -2 .. nb + 1
    c3[:2], c3[nb + 2:] = 0, 0                           # c3 of a bin outside the histogram is 0, not the window's sum (t3d.h)
    c = c3[2:2 + nb]
    ok = (c.astype(np.float64) >= o['min_share'] * float(n_finite)) & (c >= o['min_inliers']) & (c > c3[0:nb]) & (c > c3[1:nb + 1]) \
        & (c >= c3[3:nb + 3]) & (c >= c3[4:nb + 4])
    if not ok.any():
        counts[2], counts[3] = -1, abi.FLOOR_NONE
        return plane, counts, hist
    b = int(np.argmax(ok))
    counts[2] = b
    z0 = o['z_lo'] + (float(b) + 0.5) * o['bin']
    with np.errstate(invalid='ignore'):
        inl = fin & (np.abs(z - z0) <= o['band'])
    n1 = int(inl.sum())
    if n1 == 0:
        counts[3] = abi.FLOOR_NONE
        return plane, counts, hist
    xs, ys, zs = (np.where(inl, a, 0.0) for a in (x, y, z))      # (what is not an inlier is never added: this keeps NaN * 0 out)
    Sx, Sy, Sz = ordered_sums(np.stack([xs, ys, zs], 1), inl)
    dn = float(n1)
    mx, my, mz = Sx / dn, Sy / dn, Sz / dn
    dx, dy, dz = xs - mx, ys - my, zs - mz
    Sxx, Sxy, Syy, Sxz, Syz, Szz = ordered_sums(np.stack([dx * dx, dx * dy, dy * dy, dx * dz, dy * dz, dz * dz], 1), inl)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        det = np.float64(Sxx * Syy - Sxy * Sxy)
        a, bb = (Sxz * Syy - Syz * Sxy) / det, (Syz * Sxx - Sxz * Sxy) / det
        spread = (dn * o['min_spread']) * o['min_spread']
        good = np.isfinite(a) and np.isfinite(bb) and a * a + bb * bb <= o['max_slope2'] and Sxx >= spread and Syy >= spread \
            and det >= o['min_det_ratio'] * (Sxx * Syy)
    flags = 0
    if not good:
        a, bb, flags = 0.0, 0.0, abi.FLOOR_LEVEL
    r = Szz - (a * Sxz + bb * Syz)
    plane[:] = (a, bb, mz - (a * mx + bb * my), mx, my, mz, (r if r > 0.0 else 0.0) / dn, z0)
    counts[1], counts[3] = n1, flags
    return plane, counts, hist


def scene_floor_batch(points, offsets, o=OPTIONS):
    """(plane [S, 8], counts [S, 4], hist [S, n_bins]) of the scenes of `points` [sum n, ld]."""
    S = len(offsets) - 1
    out = [scene_floor(points[max(int(offsets[s]), 0):max(int(offsets[s + 1]), int(offsets[s]), 0)], o) for s in range(S)]
    if not out:
        return np.zeros((0, 8)), np.zeros((0, 4), np.int32), np.zeros((0, o['n_bins']), np.int32)
    return tuple(np.stack(c) for c in zip(*out))


def detect_floor(label, corners, scene_index, plane, counts, mode, max_snap):
    """-> (gap [n] fp64, flags [n] int32, label_out [n, 7] fp32, corners_out [n, 8, 3] fp32)."""
    label, corners = np.asarray(label, np.float32).reshape(-1, 7), np.asarray(corners, np.float32).reshape(-1, 8, 3)
    n, S = len(label), len(plane)
    idx = np.asarray(scene_index, np.int64)
    flags = np.zeros(n, np.int32)
    inside = (idx >= 0) & (idx < S)
    safe = np.where(inside, idx, 0)
    none = ~inside
    if S:
        none |= (np.asarray(counts)[safe, 3] & abi.FLOOR_NONE) != 0
    flags[none] |= abi.DETECT_FLOOR_NO_FLOOR
    flags[~np.isfinite(label).all(1)] |= abi.DETECT_FLOOR_NOT_FINITE
    live = flags == 0
    pl = np.asarray(plane, np.float64)[safe] if S else np.zeros((n, 8))
    h, tx, ty, tz = (label[:, k].astype(np.float64) for k in (0, 3, 4, 5))
    with np.errstate(invalid='ignore', over='ignore'):
        yf = -((pl[:, 0] * tx + pl[:, 1] * tz) + pl[:, 2])
        gap = yf - ty
        flags[live & (np.abs(gap) > max_snap)] |= abi.DETECT_FLOOR_TOO_FAR
        ty1 = yf.astype(np.float32)
        h1 = label[:, 0].copy()
        if mode == 2:
            h1 = (yf - (ty - h)).astype(np.float32)
            flags[live & ~(h1 > 0)] |= abi.DETECT_FLOOR_INVERTED
    if mode != 0:
        flags[live & (flags == 0)] = abi.DETECT_FLOOR_SNAPPED
    gap = gap.copy()
    gap.view(np.uint64)[~live] = NAN_BITS
    snapped = (flags & abi.DETECT_FLOOR_SNAPPED) != 0
    label_out, corners_out = label.copy(), corners.copy()
    label_out[snapped, 0], label_out[snapped, 4] = h1[snapped], ty1[snapped]
    two = np.float32(2.0)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(8):
            y = (h1 if k < 4 else -h1) / two + (ty1 - h1 / two)
            corners_out[snapped, k, 1] = y.astype(np.float32)[snapped]
    return gap, flags, label_out, corners_out


def nonneg(v):
    return v >= 0.0                                      # False for a NaN


def scene_floor_refusal(p):
    need = ('points', 'scene_offsets', 'plane', 'counts', 'hist', 'workspace')
    if any(not getattr(p, k) for k in need) or p.reserved != 0:
        return -1
    if p.n_scenes < 0 or p.n_bins < 1:
        return -1
    if not (0.0 < p.bin < np.inf) or not (0.0 < p.inv_bin < np.inf) or not p.z_hi > p.z_lo:
        return -1
    if not 0.0 <= p.min_share <= 1.0 or p.min_inliers < 0:
        return -1
    if not (nonneg(p.band) and nonneg(p.max_slope2) and nonneg(p.min_spread) and nonneg(p.min_det_ratio)):
        return -1
    if p.n_bins > abi.SCENE_FLOOR_MAX_BINS or p.ld < 3 or p.n_scenes > 65535:
        return -2
    if p.workspace % 8 or p.workspace_bytes < abi.scene_floor_workspace_bytes(p.n_scenes):
        return -1
    return 0


def detect_floor_refusal(p):
    if any(not getattr(p, k) for k in ('label', 'corners', 'scene_index', 'gap', 'flags')) or p.reserved != 0:
        return -1
    if p.n < 0 or p.n_scenes < 0 or (p.n_scenes > 0 and (not p.plane or not p.counts)):
        return -1
    if p.mode < 0 or p.mode > 2 or (p.mode != 0 and (not p.label_out or not p.corners_out)) or not nonneg(p.max_snap):
        return -1
    return 0


class FloorSpec:
    """The two entry points, to mix into a specification library."""

    def t3d_scene_floor(self, a, stream):
        if not a:
            return -1
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        rc = scene_floor_refusal(p)
        if rc or p.n_scenes == 0:
            return rc
        S = p.n_scenes
        off = arr(p.scene_offsets, S + 1)
        points = arr(p.points, max(int(off.max()), 0), p.ld)
        o = {k: getattr(p, k) for k in OPTIONS}
        plane, counts, hist = scene_floor_batch(points, off, o)
        arr(p.plane, S, 8)[:], arr(p.counts, S, 4)[:], arr(p.hist, S, p.n_bins)[:] = plane, counts, hist
        return 0

    def t3d_detect_floor(self, a, stream):
        if not a:
            return -1
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        rc = detect_floor_refusal(p)
        if rc or p.n == 0:
            return rc
        n, S = p.n, p.n_scenes
        plane = arr(p.plane, S, 8) if S else np.zeros((0, 8))
        counts = arr(p.counts, S, 4) if S else np.zeros((0, 4), np.int32)
        gap, flags, lo, co = detect_floor(arr(p.label, n, 7), arr(p.corners, n, 8, 3), arr(p.scene_index, n), plane, counts, p.mode, p.max_snap)
        arr(p.gap, n)[:], arr(p.flags, n)[:] = gap, flags
        if p.label_out:
            arr(p.label_out, n, 7)[:] = lo
        if p.corners_out:
            arr(p.corners_out, n, 8, 3)[:] = co
        return 0


class FakeFloorLib(FloorSpec, FakeSceneLib):
    pass
