"""Headless pictures of points and boxes, painted on the device (t3d_render, csrc/render.hip).

The reference's viewer needs vtk and a display.  Here a picture is a `View`: a 4x4 matrix, a size, a background, and the points, 3-D
boxes and 2-D rectangles to paint in it; `Renderer.render(views)` paints any number of views in one call of the rasteriser and copies
the finished uint8 images back once.  The coordinates of everything in a view are the matrix's own: for the builders below, upright
camera coordinates (x right, y down, z forward), which is what t3d_detect_decode writes corners in.

    image_view(Rtilt, K, H, W, image)     the scene's camera: upright camera -> depth axes -> Rtilt^T -> camera axes -> K
    bev_view(x_range, z_range, H, W)      orthographic from above, far at the top of the picture
    side_view(z_range, y_range, H, W)     orthographic from the side (looking along +x), up at the top

The rules of the rasteriser (pixel centres on integers, depth contests, the closed-form segments, the painting order) are in
include/t3d.h.  `write_png` needs zlib only.
"""
import ctypes as C
import struct
import zlib

import numpy as np
import torch

from . import abi


def _rgb(r, g, b):
    """A colour from its bytes: b / 255 converts back to exactly b, far from a rounding boundary of the byte conversion."""
    return (r / 255.0, g / 255.0, b / 255.0)


# One colour per class in constants.type2class order (bed, table, sofa, chair, toilet, desk, dresser, night_stand, bookshelf, bathtub).
CLASS_PALETTE = (_rgb(230, 25, 25), _rgb(25, 115, 230), _rgb(242, 140, 25), _rgb(153, 51, 204), _rgb(25, 191, 191),
                 _rgb(242, 217, 38), _rgb(217, 76, 153), _rgb(140, 89, 38), _rgb(76, 76, 242), _rgb(242, 153, 178))
GT_COLOUR = _rgb(25, 217, 51)                 # ground truth: green
SUPPRESSED_COLOUR = _rgb(140, 140, 140)       # a detection NMS dropped: grey
PRED_COLOUR = _rgb(255, 255, 255)             # a predicted box next to its label box (viewer): white
MASK_COLOURS = (_rgb(89, 89, 102), _rgb(242, 191, 25))      # points outside / inside a mask
# a predicted against a ground-truth mask (viewer): neither, predicted only, ground truth only, both
MASK_AGREEMENT = (_rgb(89, 89, 102), _rgb(230, 51, 51), _rgb(51, 102, 242), _rgb(51, 217, 76))
POINT_COLOUR = _rgb(204, 204, 204)
MODES = {'rgb': abi.RENDER_RGB, 'label': abi.RENDER_LABEL, 'flat': abi.RENDER_FLAT}
DEPTH_TO_CAMERA = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])      # upright depth (x, y, z) -> upright camera (x, -z, y)


def class_colour(cls):
    """cls: a class name or index."""
    from .constants import type2class
    return CLASS_PALETTE[(type2class[cls] if isinstance(cls, str) else int(cls)) % len(CLASS_PALETTE)]


class View:
    """One picture.  P: 4x4 (kept in fp64 here, rounded to fp32 for the device); image: uint8 [H,W,3] background or None (bg_colour)."""

    def __init__(self, P, H, W, w_near=0.5, image=None, bg_colour=(0.0, 0.0, 0.0)):
        self.P = np.asarray(P, np.float64).reshape(4, 4)
        self.H, self.W, self.w_near, self.bg_colour = int(H), int(W), float(w_near), tuple(bg_colour)
        if image is not None:
            image = np.ascontiguousarray(image, np.uint8)
            if image.shape != (self.H, self.W, 3):
                raise ValueError('the background is %s, the view %s' % (image.shape, (self.H, self.W, 3)))
        self.image = image
        self.point_sets, self.box_sets, self.rect_list = [], [], []

    def points(self, xyz, rgb=None, label=None, mode=None, colour0=POINT_COLOUR, colour1=MASK_COLOURS[1], splat=1):
        """xyz [n,3] (a NumPy array or a tensor on the runtime's device, any float type); rgb [n,3] in [0,1]; label [n] (non-zero: colour1).
        mode: 'rgb' / 'label' / 'flat' (default: by what is given).  The same xyz object given to several views is uploaded once."""
        mode = mode or ('rgb' if rgb is not None else 'label' if label is not None else 'flat')
        if mode not in MODES or (mode == 'rgb' and rgb is None) or (mode == 'label' and label is None):
            raise ValueError('mode %r without its array' % (mode,))
        if splat not in (1, 3, 5):
            raise ValueError('splat is 1, 3 or 5, got %r' % (splat,))
        self.point_sets.append(dict(xyz=xyz, rgb=rgb, label=label, mode=mode, colour0=tuple(colour0), colour1=tuple(colour1), splat=splat))
        return self

    def boxes(self, corners, colours, thickness=1, index=None):
        """corners [m,8,3] in get_3d_box order (NumPy or device tensor); index: the rows to draw (default: all); colours: one colour or
        one per drawn box.  Drawn in the order given, later over earlier."""
        m = int(corners.shape[0])
        index = list(range(m)) if index is None else [int(i) for i in index]
        if any(not 0 <= i < m for i in index):
            raise ValueError('a box index outside [0, %d)' % m)
        colours = [tuple(colours)] * len(index) if len(colours) == 3 and np.ndim(colours[0]) == 0 else [tuple(c) for c in colours]
        if len(colours) != len(index):
            raise ValueError('%d colours for %d boxes' % (len(colours), len(index)))
        if not 1 <= thickness <= 5:
            raise ValueError('thickness is 1..5, got %r' % (thickness,))
        self.box_sets.append(dict(corners=corners, index=index, colours=colours, thickness=int(thickness)))
        return self

    def rects(self, boxes2d, colours, thickness=1):
        """boxes2d [k,4] = (xmin, ymin, xmax, ymax) in pixels of this view."""
        boxes2d = np.asarray(boxes2d, np.float64).reshape(-1, 4)
        colours = [tuple(colours)] * len(boxes2d) if len(colours) == 3 and np.ndim(colours[0]) == 0 else [tuple(c) for c in colours]
        if len(colours) != len(boxes2d):
            raise ValueError('%d colours for %d rectangles' % (len(colours), len(boxes2d)))
        if not 1 <= thickness <= 5:
            raise ValueError('thickness is 1..5, got %r' % (thickness,))
        self.rect_list += [(tuple(b), c, int(thickness)) for b, c in zip(boxes2d, colours)]
        return self


def image_view(Rtilt, K, H, W, image=None, w_near=0.05):
    """The scene's own camera over upright camera coordinates: (x, y, z) -> depth axes (x, z, -y) -> Rtilt^T -> camera axes (x, -z, y)
    -> K, as sunrgbd_data's projection; D = W = the camera depth, so u, v index the image as the reference's box3d_pts_2d does."""
    Rtilt, K = np.asarray(Rtilt, np.float64).reshape(3, 3), np.asarray(K, np.float64).reshape(3, 3)
    M = K @ DEPTH_TO_CAMERA @ Rtilt.T @ DEPTH_TO_CAMERA.T
    P = np.zeros((4, 4))
    P[0, :3], P[1, :3], P[2, :3], P[3, :3] = M[0], M[1], M[2], M[2]
    return View(P, H, W, w_near=w_near, image=image)


def bev_view(x_range, z_range, H, W, y_top=-100.0, bg_colour=(0.0, 0.0, 0.0)):
    """Orthographic from above: x_range left to right, z_range bottom to top (far at the top); a range covers the picture edge to edge
    (pixel centres on integers: x_range[0] is u = -0.5).  W = 1; D = the height below y_top (y points down): the highest point wins."""
    (x0, x1), (z0, z1) = x_range, z_range
    P = np.zeros((4, 4))
    sx, sz = W / (x1 - x0), H / (z1 - z0)
    P[0, 0], P[0, 3] = sx, -x0 * sx - 0.5
    P[1, 2], P[1, 3] = -sz, z1 * sz - 0.5
    P[2, 1], P[2, 3] = 1.0, -y_top
    P[3, 3] = 1.0
    return View(P, H, W, w_near=0.5, bg_colour=bg_colour)


def side_view(z_range, y_range, H, W, x_near=-100.0, bg_colour=(0.0, 0.0, 0.0)):
    """Orthographic from the side, looking along +x: z_range left to right, y_range top to bottom (y points down, so up is at the top).
    W = 1; D = x - x_near: the point nearest the viewer wins."""
    (z0, z1), (y0, y1) = z_range, y_range
    P = np.zeros((4, 4))
    sz, sy = W / (z1 - z0), H / (y1 - y0)
    P[0, 2], P[0, 3] = sz, -z0 * sz - 0.5
    P[1, 1], P[1, 3] = sy, -y0 * sy - 0.5
    P[2, 0], P[2, 3] = 1.0, -x_near
    P[3, 3] = 1.0
    return View(P, H, W, w_near=0.5, bg_colour=bg_colour)


def ranges_of(xyz, pad=0.05, square=True):
    """((x0, x1), (y0, y1), (z0, z1)) of finite points [n,3] (NumPy), padded by `pad` of the extent; square: x and z get the same extent."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    xyz = xyz[np.isfinite(xyz).all(1)]
    if not len(xyz):
        return (-1.0, 1.0), (-1.0, 1.0), (0.0, 2.0)
    lo, hi = xyz.min(0), xyz.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    if square:
        ext[0] = ext[2] = max(ext[0], ext[2])
    mid = 0.5 * (lo + hi)
    lo, hi = mid - (0.5 + pad) * ext, mid + (0.5 + pad) * ext
    return (lo[0], hi[0]), (lo[1], hi[1]), (lo[2], hi[2])


def _table(cls, rows):
    t = (cls * max(len(rows), 1))()
    for i, r in enumerate(rows):
        t[i] = r
    return t


def pack_views(views, out_offsets=None):
    """-> (ctypes array of abi.RenderView, total pixels, bytes of `out`, the background bytes or None).  out_offsets: where each view's
    image starts in `out` (default: back to back)."""
    rows, bgs, at, px, bg_at = [], [], 0, 0, 0
    for i, v in enumerate(views):
        off = at if out_offsets is None else int(out_offsets[i])
        bg_off = -1
        if v.image is not None:
            bg_off = bg_at
            bgs.append(v.image.reshape(-1))
            bg_at += v.image.size
        rows.append(abi.RenderView((C.c_float * 16)(*np.asarray(v.P, np.float32).reshape(16).tolist()), v.w_near, v.H, v.W, px, off, bg_off,
                                   (C.c_float * 3)(*v.bg_colour), 0))
        px += v.H * v.W
        at = max(at, off + 3 * v.H * v.W)
    return _table(abi.RenderView, rows), px, at, (np.concatenate(bgs) if bgs else None)


def _bytes_of(table, n):
    return np.frombuffer(table, np.uint8, n * C.sizeof(table._type_)).copy() if n else np.zeros(8, np.uint8)


class Renderer:
    """Tables, workspace and output of t3d_render; `render` for views, `render_tables` for the entry point's own arguments."""

    def __init__(self, rt):
        self.rt = rt
        self.workspace = None
        self._held = ()

    def _dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.rt.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(self.rt.device)

    def render_tables(self, views, xyz, rgb, label, ranges, corners, boxes, rects, out, bg=None, total_pixels=None, total_point_items=None,
                      mirrors=True):
        """One call of t3d_render.  views / ranges / boxes / rects: ctypes arrays of abi.RenderView / RenderPoints / RenderBox /
        RenderRect with their counts as (table, n) pairs; xyz [n,3] fp32, rgb [n,3] fp32 or None, label [n] uint8 or None, corners
        [m,8,3] fp32, bg uint8 or None, out uint8: tensors on the runtime's device.  Paints into `out`; nothing is copied back.
        mirrors=False: the host copies of the tables are not handed over (only the device checks its entries)."""
        rt = self.rt
        (vt, nv), (rg, nr), (bx, nb), (rc, nc) = views, ranges, boxes, rects
        if total_pixels is None:
            total_pixels = sum(vt[i].H * vt[i].W for i in range(nv))
        if total_point_items is None:
            total_point_items = sum(rg[i].count for i in range(nr))
        self.workspace = abi.grown(self.workspace, (abi.render_workspace_bytes(max(total_pixels, 0)) + 7) // 8, torch.int64, rt.device)
        up = lambda t, n: torch.from_numpy(_bytes_of(t, n)).to(rt.device)
        d_views, d_ranges, d_boxes, d_rects = up(vt, nv), up(rg, nr), up(bx, nb), up(rc, nc)
        ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        host = lambda t, n: C.cast(t, C.c_void_p) if (mirrors and n > 0) else C.c_void_p(0)
        n_points = 0 if xyz is None else int(xyz.shape[0])
        m = 0 if corners is None else int(corners.numel() // 24)
        a = abi.RenderArgs(nv, n_points, nr, m, nb, nc, 3 if xyz is None else int(xyz.stride(0)), ptr(d_views), abi.fptr(xyz), abi.fptr(rgb),
                           abi.u8ptr(label), ptr(d_ranges), abi.fptr(corners), ptr(d_boxes), ptr(d_rects), int(total_pixels),
                           int(total_point_items), abi.u8ptr(bg), 0 if bg is None else int(bg.numel()), abi.u8ptr(out),
                           0 if out is None else int(out.numel()), ptr(self.workspace), self.workspace.numel() * 8,
                           host(vt, nv), host(rg, nr), host(bx, nb), host(rc, nc))
        self._held = (d_views, d_ranges, d_boxes, d_rects, xyz, rgb, label, corners, bg, out, vt, rg, bx, rc)      # alive until the launches have run
        self._args = a
        self.relaunch()

    def relaunch(self):
        """The launches of the last call again, on the same buffers (tools/bench_render.py times them alone)."""
        abi.check(self.rt.lib.t3d_render(C.byref(self._args), self.rt.stream()), 't3d_render')

    def gather(self, views):
        """The arguments of `render_tables` for a list of View objects -> (kwargs, bytes of out).  Arrays given to several views (or
        several times to one) are uploaded once, by identity."""
        f32 = torch.float32
        pts, pt_at, n_pts = {}, [], 0          # id(xyz) -> (first, n)
        xyz_parts, rgb_parts, lab_parts = [], [], []
        any_rgb = any(s['rgb'] is not None for v in views for s in v.point_sets)
        any_lab = any(s['label'] is not None for v in views for s in v.point_sets)
        ranges, pos = [], 0
        for vi, v in enumerate(views):
            for s in v.point_sets:
                key = (id(s['xyz']), id(s['rgb']), id(s['label']))
                if key not in pts:
                    x = self._dev(s['xyz'], f32).reshape(-1, 3)
                    n = int(x.shape[0])
                    xyz_parts.append(x)
                    if any_rgb:
                        rgb_parts.append(self._dev(s['rgb'], f32).reshape(n, 3) if s['rgb'] is not None
                                         else torch.zeros(n, 3, dtype=f32, device=self.rt.device))
                    if any_lab:
                        lab_parts.append((self._dev(s['label'], f32).reshape(n) != 0).to(torch.uint8) if s['label'] is not None
                                         else torch.zeros(n, dtype=torch.uint8, device=self.rt.device))
                    pts[key] = (n_pts, n)
                    n_pts += n
                first, n = pts[key]
                ranges.append(abi.RenderPoints(vi, first, n, MODES[s['mode']], (C.c_float * 3)(*s['colour0']), (C.c_float * 3)(*s['colour1']),
                                               s['splat'], 0, pos))
                pos += n
        cor, cor_parts, n_cor, boxes = {}, [], 0, []
        for vi, v in enumerate(views):
            for s in v.box_sets:
                if id(s['corners']) not in cor:
                    k = self._dev(s['corners'], f32).reshape(-1, 8, 3)
                    cor[id(s['corners'])] = n_cor
                    cor_parts.append(k)
                    n_cor += int(k.shape[0])
                base = cor[id(s['corners'])]
                boxes += [abi.RenderBox(vi, base + i, (C.c_float * 3)(*c), s['thickness']) for i, c in zip(s['index'], s['colours'])]
        rects = [abi.RenderRect(vi, b[0], b[1], b[2], b[3], (C.c_float * 3)(*c), t) for vi, v in enumerate(views) for b, c, t in v.rect_list]
        vt, px, out_bytes, bg = pack_views(views)
        cat = lambda parts: (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous() if parts else None
        kw = dict(views=(vt, len(views)), xyz=cat(xyz_parts), rgb=cat(rgb_parts), label=cat(lab_parts),
                  ranges=(_table(abi.RenderPoints, ranges), len(ranges)), corners=cat(cor_parts), boxes=(_table(abi.RenderBox, boxes), len(boxes)),
                  rects=(_table(abi.RenderRect, rects), len(rects)), bg=None if bg is None else torch.from_numpy(bg).to(self.rt.device),
                  total_pixels=px, total_point_items=pos)
        return kw, out_bytes

    def render(self, views):
        """-> one uint8 [H,W,3] array per view.  One call of the rasteriser, one copy back."""
        views = list(views)
        if not views:
            return []
        kw, out_bytes = self.gather(views)
        out = torch.zeros(out_bytes, dtype=torch.uint8, device=self.rt.device)
        self.render_tables(out=out, **kw)
        host = out.cpu().numpy()                     # the one copy back
        vt = kw['views'][0]
        return [host[vt[i].out_offset:vt[i].out_offset + 3 * v.H * v.W].reshape(v.H, v.W, 3).copy() for i, v in enumerate(views)]


def side_by_side(panels, gap=4, colour=(40, 40, 40)):
    """uint8 panels [H_i,W_i,3] in one row, tops aligned, `gap` pixels between them."""
    H = max(p.shape[0] for p in panels)
    W = sum(p.shape[1] for p in panels) + gap * (len(panels) - 1)
    out = np.empty((H, W, 3), np.uint8)
    out[:] = np.asarray(colour, np.uint8)
    x = 0
    for p in panels:
        out[:p.shape[0], x:x + p.shape[1]] = p
        x += p.shape[1] + gap
    return out


def contact_sheet(tiles, columns=5, gap=4, colour=(40, 40, 40)):
    """Equal-sized uint8 tiles in rows of `columns`."""
    h, w = tiles[0].shape[:2]
    columns = max(1, min(columns, len(tiles)))
    rows = (len(tiles) + columns - 1) // columns
    out = np.empty((rows * h + gap * (rows - 1), columns * w + gap * (columns - 1), 3), np.uint8)
    out[:] = np.asarray(colour, np.uint8)
    for i, t in enumerate(tiles):
        r, c = divmod(i, columns)
        out[r * (h + gap):r * (h + gap) + h, c * (w + gap):c * (w + gap) + w] = t
    return out


def write_png(path, array):
    """uint8 [H,W,3] (or [H,W]: grey) -> an 8-bit PNG, with the standard library only."""
    a = np.ascontiguousarray(array, np.uint8)
    if a.ndim == 2:
        colour_type = 0
    elif a.ndim == 3 and a.shape[2] == 3:
        colour_type = 2
    else:
        raise ValueError('an image is [H,W] or [H,W,3], got %s' % (a.shape,))
    H, W = a.shape[:2]
    raw = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, -1)], axis=1).tobytes()      # filter type 0 in front of every row

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    with open(path, 'wb') as fh:
        fh.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, colour_type, 0, 0, 0)) +
                 chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def read_png(path):
    """The inverse of write_png, for the files it writes (8-bit grey or RGB, filter 0, not interlaced)."""
    data = open(path, 'rb').read()
    if data[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError('%s is no PNG' % path)
    at, idat, head = 8, b'', None
    while at < len(data):
        n, tag = struct.unpack('>I', data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if tag == b'IHDR':
            head = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
        at += 12 + n
    W, H, depth, colour_type = head[:4]
    ch = {0: 1, 2: 3}[colour_type]
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * ch)
    if depth != 8 or rows[:, 0].any():
        raise ValueError('%s: not a file of write_png' % path)
    img = rows[:, 1:].reshape(H, W, ch)
    return img[:, :, 0].copy() if ch == 1 else img.copy()
