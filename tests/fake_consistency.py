"""NumPy fp64 specification of t3d_detect_consistency (include/t3d.h, csrc/consistency.hip): the same operations in the same order,
written elementwise (no np.dot, no reductions that may reorder a float sum), so that on equal fp32 inputs every output equals the
kernel's bit for bit -- up to the device's cos / sin where rot_angle is given (see `margins`)."""
import numpy as np

BAD_PROJECTION, EMPTY_MASK, NO_CALIB = 1, 2, 4
EDGES = (1, 3, 4)          # corner 0's neighbours in get_3d_box order: w, l, h


def frame(xyz, rot_angle):
    """The points [B, N, >= 3] in the corners' frame -> (x', y', z') fp64 [B, N] each."""
    x, y, z = (np.asarray(xyz[..., i], np.float64) for i in range(3))
    if rot_angle is None:
        return x, y, z
    rot = np.asarray(rot_angle, np.float32).astype(np.float64).reshape(-1, 1)
    c, s = np.cos(-rot), np.sin(-rot)
    return c * x - s * z, y, s * x + c * z


def edge_terms(xyz, corners, rot_angle):
    """-> (dv [3, B, N], dd [3, B, 1]): per edge the point's projection on it and the edge's squared length."""
    k = np.asarray(corners, np.float32).astype(np.float64).reshape(-1, 8, 3)
    px, py, pz = frame(xyz, rot_angle)
    q = (px - k[:, 0, 0:1], py - k[:, 0, 1:2], pz - k[:, 0, 2:3])
    dv, dd = [], []
    for j in EDGES:
        e = [k[:, j, i:i + 1] - k[:, 0, i:i + 1] for i in range(3)]
        dv.append((q[0] * e[0] + q[1] * e[1]) + q[2] * e[2])
        dd.append((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return np.stack(dv), np.stack(dd)


def margins(xyz, corners, rot_angle):
    """min over the edges of min(|dv|, |dv - dd|) / dd per point [B, N]: how far, relative to the edge, a point is from a face.  A point
    with a margin of at least 1e-9 is on the same side of every face whatever the last place of cos / sin is: |x|, |z| < 2^4 and an
    edge below 2^3 move dv by less than 2^-53 * 2^8 ~ 3e-14 per last place, far below 1e-9 * dd for any edge longer than a millimetre."""
    dv, dd = edge_terms(xyz, corners, rot_angle)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.min(np.minimum(np.abs(dv), np.abs(dv - dd)) / dd, axis=0)


def project(corners, calib_row):
    """corners [..., 3] (upright camera) -> (u, v, depth): project_upright_camera_to_upright_depth, then project_upright_depth_to_image."""
    cal = np.asarray(calib_row, np.float64)
    R, K = cal[:9].reshape(3, 3), cal[9:18].reshape(3, 3)
    k = np.asarray(corners, np.float64)
    d = (k[..., 0], k[..., 2], -k[..., 1])
    t = [(R[0, i] * d[0] + R[1, i] * d[1]) + R[2, i] * d[2] for i in range(3)]
    cam = (t[0], -t[2], t[1])
    w = [(K[i, 0] * cam[0] + K[i, 1] * cam[1]) + K[i, 2] * cam[2] for i in range(3)]
    with np.errstate(divide='ignore', invalid='ignore'):
        return w[0] / w[2], w[1] / w[2], cam[2]


def _clamp(x, hi):
    return 0.0 if x < 0.0 else (hi if x > hi else x)


def rectangle(corners, calib_row):
    """One detection's eight corners -> ((xmin, ymin, xmax, ymax) clipped where the row has an image size, bad projection?)."""
    u, v, depth = project(np.asarray(corners, np.float32).astype(np.float64).reshape(8, 3), calib_row)
    bad = False
    xmin, ymin, xmax, ymax = u[0], v[0], u[0], v[0]
    for k in range(8):
        bad = bad or bool(depth[k] <= 0.0) or not np.isfinite(u[k]) or not np.isfinite(v[k])
        xmin = u[k] if u[k] < xmin else xmin
        xmax = u[k] if u[k] > xmax else xmax
        ymin = v[k] if v[k] < ymin else ymin
        ymax = v[k] if v[k] > ymax else ymax
    if bad:
        return (0.0, 0.0, 0.0, 0.0), True
    W, H = float(calib_row[18]), float(calib_row[19])
    if W > 0.0 and H > 0.0:
        xmin, xmax, ymin, ymax = _clamp(xmin, W - 1.0), _clamp(xmax, W - 1.0), _clamp(ymin, H - 1.0), _clamp(ymax, H - 1.0)
    return (np.float64(xmin), np.float64(ymin), np.float64(xmax), np.float64(ymax)), False


def rect_iou(a, b):
    """IoU of the rectangle a with the 2-D box b, both (xmin, ymin, xmax, ymax) fp64."""
    a, b = [np.float64(v) for v in a], [np.float64(v) for v in b]
    iw = (a[2] if a[2] < b[2] else b[2]) - (a[0] if a[0] > b[0] else b[0])
    ih = (a[3] if a[3] < b[3] else b[3]) - (a[1] if a[1] > b[1] else b[1])
    inter = iw * ih if (iw > 0.0 and ih > 0.0) else np.float64(0.0)
    uni = ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter
    return inter / uni if uni > 0.0 else np.float64(0.0)


def consistency(xyz, logits, corners, rot_angle, box2d, calib_index, calib, n_valid=None, counts=None, reproj=None):
    """-> (counts [B, 4] int32: n_mask, n_box, n_both, flags; reproj [B, 5] fp64: xmin, ymin, xmax, ymax, IoU).  xyz [B, N, >= 3],
    logits [B, N, 2], corners [B, 8, 3], rot_angle [B] or None: fp32 values; box2d [B, 4], calib [n_calib, 20] fp64.  Rows at or past
    n_valid keep what `counts` / `reproj` held (zeros by default)."""
    logits = np.asarray(logits, np.float32)
    B = logits.shape[0]
    n = B if n_valid is None else max(0, min(B, int(n_valid)))
    counts = np.zeros((B, 4), np.int32) if counts is None else np.array(counts, np.int32)
    reproj = np.zeros((B, 5), np.float64) if reproj is None else np.array(reproj, np.float64)
    calib = np.asarray(calib, np.float64).reshape(-1, 20)
    if n == 0:
        return counts, reproj
    mask = logits[:n, :, 1] > logits[:n, :, 0]
    dv, dd = edge_terms(np.asarray(xyz)[:n], np.asarray(corners)[:n], None if rot_angle is None else np.asarray(rot_angle)[:n])
    with np.errstate(invalid='ignore'):
        inside = np.all((0.0 <= dv) & (dv <= dd), axis=0)
    for b in range(n):
        n_mask, n_box, n_both = int(mask[b].sum()), int(inside[b].sum()), int((mask[b] & inside[b]).sum())
        flags = EMPTY_MASK if n_mask == 0 else 0
        ci = int(calib_index[b])
        r = (0.0, 0.0, 0.0, 0.0, 0.0)
        if not 0 <= ci < len(calib):
            flags |= NO_CALIB
        else:
            rect, bad = rectangle(np.asarray(corners)[b], calib[ci])
            if bad:
                flags |= BAD_PROJECTION
            else:
                r = rect + (rect_iou(rect, box2d[b]),)
        counts[b] = (n_mask, n_box, n_both, flags)
        reproj[b] = r
    return counts, reproj


class ConsistencySpec:
    """Mix-in: t3d_detect_consistency for a specification library (FakeLib and its subclasses), behind the ctypes struct on host pointers."""

    def t3d_detect_consistency(self, a, stream):
        import ctypes as C
        from fake_t3d import AbiSizeError, _struct, arr
        if not a:
            return -1
        try:
            p = _struct(a)
        except AbiSizeError:
            return -4
        B, N = p.B, p.N
        if B <= 0 or N <= 0 or p.n_valid < 0 or p.ld_xyz < 3 or p.n_calib < 0:
            return -2
        if not all((p.xyz, p.logits, p.corners, p.box2d, p.calib_index, p.calib, p.counts, p.reproj)):
            return -1
        if C.cast(p.logits, C.c_void_p).value & 7:
            return -1
        n = min(B, p.n_valid)
        if n == 0:
            return 0
        calib = arr(p.calib, p.n_calib, 20) if p.n_calib else np.zeros((0, 20))
        counts, reproj = consistency(arr(p.xyz, B, N, p.ld_xyz)[:n], arr(p.logits, B, N, 2)[:n], arr(p.corners, B, 8, 3)[:n],
                                     arr(p.rot_angle, B)[:n] if p.rot_angle else None, arr(p.box2d, B, 4)[:n], arr(p.calib_index, B)[:n], calib)
        arr(p.counts, B, 4)[:n] = counts
        arr(p.reproj, B, 5)[:n] = reproj
        return 0
