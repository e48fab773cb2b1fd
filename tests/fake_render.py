"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_render (include/t3d.h, csrc/render.hip), on the fp32-rounded
inputs: `render_arrays` is the rule on arrays and Python tables, RenderSpec the entry point behind the ctypes struct on host pointers,
so that render.Renderer and detect --vis_dir run end to end through Runtime(device='cpu', lib=FakeRenderLib()).

The pieces the shared cases (render_check.py) need for their repair rule are functions of their own: `project`, `round_px`,
`box_edges`, `rect_edges`, `segment_pixels`, `colour_value`."""
import ctypes as C
import math

import numpy as np

from fake_nms import DetectNmsSpec
from fake_detect import DetectDecodeSpec
from fake_t3d import AbiSizeError, FakeLib, _struct, arr
from transferable3d_amd import abi

RGB, LABEL, FLAT = 0, 1, 2
PIX_CLAMP = 1 << 20
EDGES = [(i, (i + 1) % 4) for i in range(4)] + [(4 + i, 4 + (i + 1) % 4) for i in range(4)] + [(i, i + 4) for i in range(4)]


def project(P, xyz):
    """(X, Y, D, W) [n] each, fp64, of fp32 points under the fp32 matrix P."""
    P = np.asarray(P, np.float32).astype(np.float64).reshape(4, 4)
    x = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        h = x[:, 0:1] * P[:, 0] + x[:, 1:2] * P[:, 1] + x[:, 2:3] * P[:, 2] + P[:, 3]
    return h[:, 0], h[:, 1], h[:, 2], h[:, 3]


def round_px(u):
    return np.floor(np.asarray(u, np.float64) + 0.5)


def colour_value(c):
    """c*255 + 0.5 of an fp32 colour component, fp64: the byte is its floor, clamped to [0, 255] (a NaN: 0)."""
    return np.asarray(c, np.float32).astype(np.float64) * 255.0 + 0.5


def to_byte(c):
    v = np.floor(colour_value(c))
    return np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 255.0)).astype(np.uint8)


def segment_pixels(ax, ay, bx, by):
    """The pixel set of a segment between two integer pixels -> [(x, y)], t3d.h's closed form in Python integers."""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    x_major = abs(bx - ax) >= abs(by - ay)
    a, b = ((ax, ay), (bx, by)) if x_major else ((ay, ax), (by, bx))
    if b < a:                                        # the smaller major coordinate, then the smaller minor one
        a, b = b, a
    d_maj, d_min = b[0] - a[0], b[1] - a[1]
    out = []
    for m in range(a[0], b[0] + 1):
        mn = a[1] if d_maj == 0 else a[1] + (2 * (m - a[0]) * d_min + d_maj) // (2 * d_maj)      # (// floors)
        out.append((m, mn) if x_major else (mn, m))
    return out


def clip_to_near(pa, pb, w_near):
    """pa, pb: (X, Y, W) -> (ua, va, ub, vb) after the near-plane rule, or None (both behind, or a non-finite pixel coordinate)."""
    (Xa, Ya, Wa), (Xb, Yb, Wb) = pa, pb
    behind_a, behind_b = Wa < w_near, Wb < w_near
    if behind_a and behind_b:
        return None
    with np.errstate(all='ignore'):
        if behind_a or behind_b:
            t = (w_near - Wa) / (Wb - Wa)
            Xc, Yc = Xa + t * (Xb - Xa), Ya + t * (Yb - Ya)
            if behind_a:
                Xa, Ya, Wa = Xc, Yc, w_near
            else:
                Xb, Yb, Wb = Xc, Yc, w_near
        uv = (np.float64(Xa) / Wa, np.float64(Ya) / Wa, np.float64(Xb) / Wb, np.float64(Yb) / Wb)
    return uv if all(math.isfinite(v) for v in uv) else None


def box_edges(P, w_near, corners8):
    """The 12 edges of one box -> [(ua, va, ub, vb) or None] (all None: a non-finite corner drops the box)."""
    X, Y, D, W = project(P, corners8)
    if not (np.isfinite(X).all() and np.isfinite(Y).all() and np.isfinite(D).all() and np.isfinite(W).all()):
        return [None] * 12
    wn = float(np.float32(w_near))
    return [clip_to_near((X[i], Y[i], W[i]), (X[j], Y[j], W[j]), wn) for i, j in EDGES]


def rect_edges(xmin, ymin, xmax, ymax):
    c = [float(np.float32(v)) for v in (xmin, ymin, xmax, ymax)]
    if not all(math.isfinite(v) for v in c):
        return [None] * 4
    x0, y0, x1, y1 = c
    return [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]


def stamp(ordinals, edge, thickness, ordinal, H, W):
    if edge is None:
        return
    ax, ay, bx, by = [int(np.clip(round_px(v), -PIX_CLAMP, PIX_CLAMP)) for v in edge]
    lo, hi = -((thickness - 1) // 2), thickness // 2
    # the steps whose stamp can reach the view (what lies farther out paints nothing: the walk need not visit it)
    x_major = abs(bx - ax) >= abs(by - ay)
    if max(ax, bx) < -hi or max(ay, by) < -hi or min(ax, bx) > W - 1 - lo or min(ay, by) > H - 1 - lo:
        return
    if max(abs(ax), abs(ay), abs(bx), abs(by)) > 4 * (H + W):      # a long segment: walk only the major range that can touch the view
        a, b = ((ax, ay), (bx, by)) if x_major else ((ay, ax), (by, bx))
        if b < a:
            a, b = b, a
        n_maj = W if x_major else H
        d_maj, d_min = b[0] - a[0], b[1] - a[1]
        pix = []
        for m in range(max(a[0], -hi), min(b[0], n_maj - 1 - lo) + 1):
            mn = a[1] if d_maj == 0 else a[1] + (2 * (m - a[0]) * d_min + d_maj) // (2 * d_maj)
            pix.append((m, mn) if x_major else (mn, m))
    else:
        pix = segment_pixels(ax, ay, bx, by)
    for x, y in pix:
        x0, x1, y0, y1 = max(x + lo, 0), min(x + hi, W - 1), max(y + lo, 0), min(y + hi, H - 1)
        if x0 <= x1 and y0 <= y1:
            ordinals[y0:y1 + 1, x0:x1 + 1] = np.maximum(ordinals[y0:y1 + 1, x0:x1 + 1], ordinal)


def point_winners(view, xyz, ranges):
    """Per pixel of one view, the index (in the point array) of the winning point, -1 for none, and the range that colours it.
    ranges: [(table position, dict)] of this view."""
    H, W = view['H'], view['W']
    cand_pix, cand_D, cand_idx = [], [], []
    wn = float(np.float32(view['w_near']))
    for _, r in ranges:
        idx = np.arange(r['first'], r['first'] + r['count'])
        if not len(idx):
            continue
        X, Y, D, Wc = project(view['P'], xyz[idx])
        with np.errstate(all='ignore'):
            ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(D) & np.isfinite(Wc) & (Wc >= wn) & (D >= 0)
            u, v = X / Wc, Y / Wc
            ok &= np.isfinite(u) & np.isfinite(v)
            px, py = round_px(np.where(ok, u, 0)), round_px(np.where(ok, v, 0))
        ok &= (px >= -4) & (px <= W + 4) & (py >= -4) & (py <= H + 4)
        px, py, D, idx = px[ok].astype(np.int64), py[ok].astype(np.int64), D[ok] + 0.0, idx[ok]
        h = r['splat'] // 2
        for dy in range(-h, h + 1):
            for dx in range(-h, h + 1):
                x, y = px + dx, py + dy
                inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                cand_pix.append((y * W + x)[inside])
                cand_D.append(D[inside])
                cand_idx.append(idx[inside])
    winner = np.full(H * W, -1, np.int64)
    if cand_pix:
        pix, D, idx = np.concatenate(cand_pix), np.concatenate(cand_D), np.concatenate(cand_idx)
        order = np.lexsort((idx, D, pix))
        pix, idx = pix[order], idx[order]
        first = np.concatenate([[True], pix[1:] != pix[:-1]]) if len(pix) else np.zeros(0, bool)
        winner[pix[first]] = idx[first]
    return winner.reshape(H, W)


def point_colours(winner, view_ranges, rgb, label):
    """[H,W,3] uint8 and [H,W] bool (painted) from the winners of one view."""
    H, W = winner.shape
    img, painted = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), bool)
    for _, r in reversed(view_ranges):                 # the first range in table order that holds the index colours it: paint it last
        m = (winner >= r['first']) & (winner < r['first'] + r['count'])
        if not m.any():
            continue
        idx = winner[m]
        if r['mode'] == RGB:
            col = to_byte(rgb[idx])
        elif r['mode'] == LABEL:
            col = np.where((label[idx] != 0)[:, None], to_byte(r['colour1'])[None], to_byte(r['colour0'])[None])
        else:
            col = np.broadcast_to(to_byte(r['colour0']), (len(idx), 3))
        img[m], painted[m] = col, True
    return img, painted


def render_arrays(views, xyz, rgb, label, ranges, corners, boxes, rects, out, bg=None):
    """The rule on arrays.  views: [{'P', 'w_near', 'H', 'W', 'out_offset', 'bg_offset', 'bg_colour'}]; ranges: [{'view', 'first',
    'count', 'mode', 'colour0', 'colour1', 'splat'}]; boxes: [{'view', 'box', 'colour', 'thickness'}]; rects: [{'view', 'xmin', 'ymin',
    'xmax', 'ymax', 'colour', 'thickness'}]; out, bg: flat uint8 arrays.  Paints into `out` in place (entries are valid: the caller
    checked them)."""
    for vi, v in enumerate(views):
        H, W = v['H'], v['W']
        if v['bg_offset'] >= 0:
            img = np.array(bg[v['bg_offset']:v['bg_offset'] + 3 * H * W]).reshape(H, W, 3)
        else:
            img = np.broadcast_to(to_byte(v['bg_colour']), (H, W, 3)).copy()
        mine = [(k, r) for k, r in enumerate(ranges) if r['view'] == vi]
        if mine:
            winner = point_winners(v, xyz, mine)
            col, painted = point_colours(winner, mine, rgb, label)
            img[painted] = col[painted]
        ordinals = np.zeros((H, W), np.int64)
        for k, b in enumerate(boxes):
            if b['view'] == vi:
                for e in box_edges(v['P'], v['w_near'], corners[b['box']]):
                    stamp(ordinals, e, b['thickness'], 1 + k, H, W)
        for k, r in enumerate(rects):
            if r['view'] == vi:
                for e in rect_edges(r['xmin'], r['ymin'], r['xmax'], r['ymax']):
                    stamp(ordinals, e, r['thickness'], 1 + len(boxes) + k, H, W)
        for o in np.unique(ordinals[ordinals > 0]):
            c = boxes[o - 1]['colour'] if o - 1 < len(boxes) else rects[o - 1 - len(boxes)]['colour']
            img[ordinals == o] = to_byte(c)
        out[v['out_offset']:v['out_offset'] + 3 * H * W] = img.reshape(-1)
    return out


def check_tables(p, views, ranges, boxes, rects):
    """What csrc/render.hip's check of the host mirrors answers: 0 or T3D_ERR_ARG.  Tables as lists of ctypes structs."""
    at = 0
    for w in views:
        if w.H <= 0 or w.W <= 0 or w.pixel_first != at or w.out_offset < 0 or w.out_offset + 3 * w.H * w.W > p.out_bytes:
            return -1
        if w.bg_offset < -1 or (w.bg_offset >= 0 and (not p.bg or w.bg_offset + 3 * w.H * w.W > p.bg_bytes)):
            return -1
        at += w.H * w.W
    if at != p.total_pixels:
        return -1
    at = 0
    for g in ranges:
        if not 0 <= g.view < p.n_views or g.first < 0 or g.count < 0 or g.first + g.count > p.n_points or g.pos_first != at:
            return -1
        if g.splat not in (1, 3, 5) or g.mode not in (RGB, LABEL, FLAT) or (g.mode == RGB and not p.rgb) or (g.mode == LABEL and not p.label):
            return -1
        at += g.count
    if at != p.total_point_items:
        return -1
    for e in boxes:
        if not 0 <= e.view < p.n_views or not 0 <= e.box < p.n_corner_boxes or not 1 <= e.thickness <= 5:
            return -1
    for e in rects:
        if not 0 <= e.view < p.n_views or not 1 <= e.thickness <= 5:
            return -1
    return 0


class RenderSpec:
    """Mix-in: t3d_render for a specification library (FakeLib and its subclasses).  The tables are read where the device pointers
    point (host memory under Runtime(device='cpu')); the mirrors, where given, are checked as the library checks them."""

    def t3d_render(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if min(p.n_views, p.n_points, p.n_ranges, p.n_corner_boxes, p.n_boxes, p.n_rects, p.total_pixels, p.total_point_items, p.ld_xyz) < 0:
            return -1
        if p.n_views == 0:
            return 0
        if not (p.views and p.out and p.workspace) or p.total_pixels == 0:
            return -1
        if (p.n_ranges > 0 and not (p.ranges and p.xyz and p.ld_xyz >= 3)) or (p.n_boxes > 0 and not (p.boxes and p.corners)) or \
                (p.n_rects > 0 and not p.rects) or (p.n_ranges == 0 and p.total_point_items != 0):
            return -1
        if p.total_pixels > 0x7fffffff:
            return -2
        if p.workspace_bytes < abi.render_workspace_bytes(p.total_pixels) or p.workspace % 8:
            return -1
        rows = lambda address, cls, n: [] if n == 0 else [C.cast(C.c_void_p(address), C.POINTER(cls))[i] for i in range(n)]
        mirrors = [rows(getattr(p, k), cls, n) if getattr(p, k) else None
                   for k, cls, n in (('views_host', abi.RenderView, p.n_views), ('ranges_host', abi.RenderPoints, p.n_ranges),
                                     ('boxes_host', abi.RenderBox, p.n_boxes), ('rects_host', abi.RenderRect, p.n_rects))]
        tables = [rows(p.views, abi.RenderView, p.n_views), rows(p.ranges, abi.RenderPoints, p.n_ranges),
                  rows(p.boxes, abi.RenderBox, p.n_boxes), rows(p.rects, abi.RenderRect, p.n_rects)]
        # (a table without a mirror is read where it lies: the specification asks for valid entries, the device skips the others)
        held = [m if m is not None else t for m, t in zip(mirrors, tables)]
        given = check_tables(p, *held)
        if given != 0:
            if any(m is not None for m in mirrors):
                return -1
            raise AssertionError('a table entry breaks the contract of t3d_render and no host mirror was given')
        col = lambda c: np.array([c[0], c[1], c[2]], np.float32)
        views = [dict(P=np.array(list(w.P), np.float32).reshape(4, 4), w_near=w.w_near, H=w.H, W=w.W, out_offset=w.out_offset,
                      bg_offset=w.bg_offset, bg_colour=col(w.bg_colour)) for w in tables[0]]
        ranges = [dict(view=g.view, first=g.first, count=g.count, mode=g.mode, colour0=col(g.colour0), colour1=col(g.colour1), splat=g.splat)
                  for g in tables[1]]
        boxes = [dict(view=b.view, box=b.box, colour=col(b.colour), thickness=b.thickness) for b in tables[2]]
        rects = [dict(view=r.view, xmin=r.xmin, ymin=r.ymin, xmax=r.xmax, ymax=r.ymax, colour=col(r.colour), thickness=r.thickness)
                 for r in tables[3]]
        xyz = arr(p.xyz, p.n_points, p.ld_xyz)[:, :3] if p.xyz and p.n_points else np.zeros((0, 3), np.float32)
        rgb = arr(p.rgb, p.n_points, 3) if p.rgb and p.n_points else None
        label = arr(p.label, p.n_points) if p.label and p.n_points else None
        corners = arr(p.corners, p.n_corner_boxes, 8, 3) if p.corners and p.n_corner_boxes else np.zeros((0, 8, 3), np.float32)
        render_arrays(views, xyz, rgb, label, ranges, corners, boxes, rects, arr(p.out, p.out_bytes), arr(p.bg, p.bg_bytes) if p.bg else None)
        return 0


class FakeRenderLib(RenderSpec, DetectNmsSpec, DetectDecodeSpec, FakeLib):
    pass
