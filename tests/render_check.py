"""Shared cases of the t3d_render tests: the CPU tests run them through the NumPy specification library (fake_render), the GPU tests
through libt3d.so, and both compare the whole output buffer, byte for byte, with fake_render.render_arrays.

The kernel decides in fp32, the specification in fp64, so no case may sit on a decision boundary.  `Case.repair()` redraws every
primitive that is closer to one than a margin, and the margins are bounds of the fp32 error of the operation sequence include/t3d.h
documents, taken from the largest intermediates of the case, times 8.  With eps = 2^-24 (the unit roundoff of fp32, every operation
rounds to nearest), first order in eps:

  Transform    a component ((p0*x + p1*y) + p2*z) + p3 passes every term through at most 4 roundings, so its error is at most
               4 eps A_r, A_r = the largest |p0 x| + |p1 y| + |p2 z| + |p3| of row r over the primitives of the case:
               E_xy = 4 eps max(A_X, A_Y), E_d = 4 eps A_D, E_w = 4 eps A_W.
  Visibility   W against w_near: margin 8 E_w.  D against 0: margin 8 E_d.
  Depth        two points contesting a pixel compare their D, each off by E_d: margin 8 * 2 E_d.  (Two points of bitwise equal
               coordinates have bitwise equal D on both sides: the index decides, by rule, and they are exempt.)
  Pixels       u = X / W: |du| <= E_xy / |W| + |u| E_w / |W| + eps |u| (the division), and u + 0.5 adds eps (|u| + 0.5).  With w_min the
               smallest |W| and U the largest |u|, |v| among the visible points that can reach the view (within 8 pixels of it; the
               others cannot, whatever their last bit):  E_u = (E_xy + U E_w) / w_min + 2 eps (U + 1).  Margin 8 E_u on the distance of
               u + 0.5 (v + 0.5) from an integer.  The same formula over the box corners in front of the near plane, with their own
               w_min and U (every |u| below the 2^20 clamp counts: a far endpoint steers the whole segment).
  Near plane   t = (w_near - Wa) / (Wb - Wa): the numerator is off by E_w + eps |num|, the denominator by 2 E_w + eps |den|, 0 <= t <= 1,
               so |dt| <= 3 E_w / |den| + 3 eps.  Xc = Xa + t (Xb - Xa): |dXc| <= 3 E_xy + |Xb - Xa| (|dt| + 2 eps) + eps |Xc|.  u = Xc /
               w_near (W = w_near exactly) and the rounding as above: with G the largest |Xb - Xa|, |Yb - Ya|, den_min the smallest |Wb -
               Wa| and U_c the largest |u| of the clipped edges,
               E_c = (3 E_xy + G (3 E_w / den_min + 5 eps)) / w_near + 3 eps (U_c + 1).
               The segment margin is 8 max(E_u of the corners, E_c).
  Rectangles   their corners are pixel coordinates already: only u + 0.5 rounds, eps (|u| + 0.5); margin 8 of that.
  Colours      c * 255 + 0.5: two roundings of a value of at most 255 c_max + 0.5; margin 8 * 2 eps (255 c_max + 0.5) on the distance
               from an integer.

A redrawn primitive is drawn again by the generator that drew it; a hand-built one cannot be and fails the case.  At most MAX_REDRAWN
(5 %, the suite's figure) of a case's primitives (points + boxes + rectangles) may be redrawn.

Every case has two views of different sizes in one call, 64 x 48 and 33 x 17, at most 2000 points and 6 box entries per view; the views lie in
`out` with gaps before, between and behind them, which hold a fill pattern that must survive."""
import ctypes as C
import functools
import os

import numpy as np
import torch

import fake_render as FR
from transferable3d_amd import abi, render as R

EPS = 2.0 ** -24
SAFETY = 8.0
MAX_REDRAWN = 0.05
SIZES = ((48, 64), (17, 33))            # (H, W) of the two views
GAPS = (5, 11, 7)                       # bytes of `out` before the first view, between the two, behind the second
ORTHO = np.eye(4)                       # u = x, v = y, D = z, W = 1
NEAR = 8                                # pixels around a view inside which a point's rounding can matter


def ortho(sx=1.0, sy=1.0, tx=0.0, ty=0.0):
    P = np.eye(4)
    P[0, 0], P[1, 1], P[0, 3], P[1, 3] = sx, sy, tx, ty
    return P


def pinhole(f, cx, cy):
    """X = f x + cx z, Y = f y + cy z, D = W = z."""
    P = np.zeros((4, 4))
    P[0, 0], P[0, 2], P[1, 1], P[1, 2], P[2, 2], P[3, 2] = f, cx, f, cy, 1.0, 1.0
    return P


def fill_pattern(n):
    return ((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8)


def colour_of(k):
    """Distinct colours from bytes (b / 255 converts back to b: far from a rounding boundary)."""
    return ((40 + 53 * k) % 256 / 255.0, (200 + 101 * k) % 256 / 255.0, (90 + 29 * k) % 256 / 255.0)


class Case:
    def __init__(self, name, seed=0, P=(ORTHO, ORTHO), w_near=(0.5, 0.5), images=(None, None), bg_colours=((0.0, 0.0, 0.0), (16 / 255.0, 32 / 255.0, 48 / 255.0)),
                 sizes=SIZES):
        self.name, self.r = name, np.random.RandomState(seed)
        self.views = [dict(P=np.asarray(P[i], np.float32).reshape(4, 4), w_near=float(np.float32(w_near[i])), H=sizes[i][0], W=sizes[i][1],
                           image=images[i], bg_colour=tuple(bg_colours[i])) for i in range(len(P))]
        self.xyz, self.rgb, self.label, self.draw_pt = [], [], [], []
        self.ranges, self.corners, self.draw_box, self.boxes, self.rects, self.draw_rect = [], [], [], [], [], []
        self.redrawn = 0

    # ---- building ----
    def add_points(self, view, pts, draw=None, mode=FR.FLAT, colour0=colour_of(1), colour1=colour_of(2), splat=1):
        """pts [n,3] -> the range.  draw(r) -> one point of the same distribution, for redraws (None: hand-built)."""
        pts = np.asarray(pts, np.float64).reshape(-1, 3)
        first = len(self.xyz)
        for p in pts:
            self.xyz.append(p)
            self.rgb.append(self.r.uniform(0, 1, 3))
            self.label.append(int(self.r.randint(0, 2)))
            self.draw_pt.append(draw)
        return self.add_range(view, first, len(pts), mode, colour0, colour1, splat)

    def add_range(self, view, first, count, mode=FR.FLAT, colour0=colour_of(1), colour1=colour_of(2), splat=1):
        self.ranges.append(dict(view=view, first=first, count=count, mode=mode, colour0=tuple(colour0), colour1=tuple(colour1), splat=splat))
        return self.ranges[-1]

    def add_box(self, view, corners8, colour, thickness=1, draw=None):
        self.corners.append(np.asarray(corners8, np.float64).reshape(8, 3))
        self.draw_box.append(draw)
        self.boxes.append(dict(view=view, box=len(self.corners) - 1, colour=tuple(colour), thickness=thickness))

    def add_segment(self, view, a, b, colour, thickness=1, z=1.0):
        """One segment a -> b (pixel coordinates under the orthographic views) as a box whose corners 0-3 are a and 4-7 are b: eight
        zero-length edges at the ends and four times the segment."""
        k = np.array([[a[0], a[1], z]] * 4 + [[b[0], b[1], z]] * 4, np.float64)
        self.add_box(view, k, colour, thickness)

    def add_rect(self, view, xmin, ymin, xmax, ymax, colour, thickness=1, draw=None):
        self.rects.append(dict(view=view, xmin=xmin, ymin=ymin, xmax=xmax, ymax=ymax, colour=tuple(colour), thickness=thickness))
        self.draw_rect.append(draw)

    # ---- arrays ----
    @property
    def n_primitives(self):
        return len(self.xyz) + len(self.boxes) + len(self.rects)

    def arrays(self):
        """(xyz [n,3] fp32, rgb [n,3] fp32, label [n] uint8, corners [m,8,3] fp32)"""
        f = lambda rows, shape: np.asarray(rows, np.float32).reshape(shape) if rows else np.zeros((0,) + shape[1:], np.float32)
        return (f(self.xyz, (-1, 3)), f(self.rgb, (-1, 3)), np.asarray(self.label, np.uint8).reshape(-1), f(self.corners, (-1, 8, 3)))

    def layout(self):
        """(out offsets of the two views, bytes of out, background offsets, background bytes or None)"""
        offs, at = [], GAPS[0]
        for i, v in enumerate(self.views):
            offs.append(at)
            at += 3 * v['H'] * v['W'] + GAPS[1 + (i + 1 == len(self.views))]
        bg_offs, bgs, b = [], [], 3                      # (the backgrounds do not start at byte 0 either)
        for v in self.views:
            if v['image'] is None:
                bg_offs.append(-1)
            else:
                bg_offs.append(b)
                bgs.append(v['image'].reshape(-1))
                b += v['image'].size + 2
        bg = None
        if bgs:
            bg = np.zeros(b, np.uint8)
            for o, img in zip([o for o in bg_offs if o >= 0], bgs):
                bg[o:o + img.size] = img
        return offs, at, bg_offs, bg

    def spec_views(self):
        offs, _, bg_offs, _ = self.layout()
        return [dict(v, out_offset=offs[i], bg_offset=bg_offs[i]) for i, v in enumerate(self.views)]

    def expected(self):
        """The whole `out` buffer of the specification, gaps included."""
        xyz, rgb, label, corners = self.arrays()
        _, n, _, bg = self.layout()
        return FR.render_arrays(self.spec_views(), xyz, rgb, label, self.ranges, corners, self.boxes, self.rects, fill_pattern(n), bg)

    # ---- the margin rule ----
    def margins(self):
        """dict of the margins of the module docstring, from the case as it stands."""
        xyz, rgb, label, corners = self.arrays()
        A = dict(xy=0.0, d=0.0, w=0.0)
        pt = dict(w_min=np.inf, U=0.0)
        co = dict(w_min=np.inf, U=0.0)
        clip = dict(G=0.0, den_min=np.inf, U=0.0, wn=np.inf, any=False)
        rect_U = max([abs(float(np.float32(r[k]))) for r in self.rects for k in ('xmin', 'ymin', 'xmax', 'ymax') if np.isfinite(r[k])] or [0.0])

        def rows(P, x):
            P, x = P.astype(np.float64), x.astype(np.float64)
            x = x[np.isfinite(x).all(1)]
            if not len(x):
                return
            a = np.abs(x[:, 0:1] * P[:, 0]) + np.abs(x[:, 1:2] * P[:, 1]) + np.abs(x[:, 2:3] * P[:, 2]) + np.abs(P[:, 3])
            A['xy'], A['d'], A['w'] = max(A['xy'], a[:, :2].max()), max(A['d'], a[:, 2].max()), max(A['w'], a[:, 3].max())

        for vi, v in enumerate(self.views):
            for r in self.ranges:
                if r['view'] != vi or not r['count']:
                    continue
                x = xyz[r['first']:r['first'] + r['count']]
                rows(v['P'], x)
                X, Y, D, W = FR.project(v['P'], x)
                with np.errstate(all='ignore'):
                    vis = np.isfinite(X + Y + D + W) & (W >= v['w_near'])
                    u, w = X / W, Y / W
                    near = vis & (u > -NEAR) & (u < v['W'] + NEAR) & (w > -NEAR) & (w < v['H'] + NEAR)
                if near.any():
                    pt['w_min'] = min(pt['w_min'], np.abs(W[near]).min())
                    pt['U'] = max(pt['U'], np.abs(u[near]).max(), np.abs(w[near]).max())
            for b in self.boxes:
                if b['view'] != vi:
                    continue
                k = corners[b['box']]
                if not np.isfinite(k).all():
                    continue
                rows(v['P'], k)
                X, Y, D, W = FR.project(v['P'], k)
                front = W >= v['w_near']
                if front.any():
                    co['w_min'] = min(co['w_min'], np.abs(W[front]).min())
                    uu = np.concatenate([X[front] / W[front], Y[front] / W[front]])
                    co['U'] = max(co['U'], np.abs(uu[np.abs(uu) < FR.PIX_CLAMP]).max(initial=0.0))
                for (i, j), e in zip(FR.EDGES, FR.box_edges(v['P'], v['w_near'], k)):
                    if e is not None and (W[i] < v['w_near']) != (W[j] < v['w_near']):
                        clip['any'] = True
                        clip['G'] = max(clip['G'], abs(X[j] - X[i]), abs(Y[j] - Y[i]))
                        clip['den_min'] = min(clip['den_min'], abs(W[j] - W[i]))
                        clip['wn'] = min(clip['wn'], v['w_near'])
                        clip['U'] = max(clip['U'], max(abs(t) for t in e if abs(t) < FR.PIX_CLAMP) if any(abs(t) < FR.PIX_CLAMP for t in e) else 0.0)
        E_xy, E_d, E_w = 4 * EPS * A['xy'], 4 * EPS * A['d'], 4 * EPS * A['w']
        e_u = lambda s: 0.0 if not np.isfinite(s['w_min']) else (E_xy + s['U'] * E_w) / s['w_min'] + 2 * EPS * (s['U'] + 1)
        e_c = 0.0 if not clip['any'] else (3 * E_xy + clip['G'] * (3 * E_w / clip['den_min'] + 5 * EPS)) / clip['wn'] + 3 * EPS * (clip['U'] + 1)
        cols = [c for r in self.ranges for c in r['colour0'] + r['colour1']] + [c for b in self.boxes + self.rects for c in b['colour']] + \
               [c for v in self.views for c in v['bg_colour']] + [1.0]
        m = dict(w=SAFETY * E_w, d0=SAFETY * E_d, dpair=SAFETY * 2 * E_d, px=SAFETY * e_u(pt), seg=SAFETY * max(e_u(co), e_c),
                 rect=SAFETY * EPS * (rect_U + 0.5), colour=SAFETY * 2 * EPS * (255 * max(abs(float(c)) for c in cols) + 0.5))
        assert max(m['px'], m['seg'], m['rect'], m['colour']) < 0.125, (self.name, m)      # (a margin near half a pixel would leave no room at all)
        return m

    def bad_primitives(self):
        """(points, boxes, rectangles) that sit inside a margin; asserts that no table colour does."""
        xyz, rgb, label, corners = self.arrays()
        m = self.margins()
        on_edge = lambda t, margin: np.abs(t - np.round(t)) < margin            # the distance of u + 0.5 (or c*255 + 0.5) from an integer
        bad_pt, bad_box, bad_rect = set(), set(), set()
        for c in [c for r in self.ranges for c in r['colour0'] + r['colour1']] + [c for b in self.boxes + self.rects for c in b['colour']] + \
                 [c for v in self.views for c in v['bg_colour']]:
            assert not on_edge(FR.colour_value(c), m['colour']), '%s: a table colour %r sits on a rounding boundary' % (self.name, c)
        for vi, v in enumerate(self.views):
            H, W_ = v['H'], v['W']
            cand = []
            for r in self.ranges:
                if r['view'] != vi or not r['count']:
                    continue
                idx = np.arange(r['first'], r['first'] + r['count'])
                X, Y, D, W = FR.project(v['P'], xyz[idx])
                with np.errstate(all='ignore'):
                    fin = np.isfinite(X + Y + D + W)
                    bad = fin & (np.abs(W - v['w_near']) < m['w'])
                    vis = fin & (W >= v['w_near'])
                    bad |= vis & (np.abs(D) < m['d0'])
                    vis &= D >= 0
                    u, w = X / W, Y / W
                    near = vis & (u > -NEAR) & (u < W_ + NEAR) & (w > -NEAR) & (w < H + NEAR)
                    bad |= near & (on_edge(u + 0.5, m['px']) | on_edge(w + 0.5, m['px']))
                    if r['mode'] == FR.RGB:
                        bad |= near & on_edge(FR.colour_value(rgb[idx]), m['colour']).any(1)
                bad_pt |= set(idx[bad].tolist())
                keep = near & ~bad
                px, py, h = FR.round_px(u[keep]).astype(np.int64), FR.round_px(w[keep]).astype(np.int64), r['splat'] // 2
                for dy in range(-h, h + 1):
                    for dx in range(-h, h + 1):
                        x, y = px + dx, py + dy
                        inside = (x >= 0) & (x < W_) & (y >= 0) & (y < H)
                        cand.append(np.stack([(y * W_ + x)[inside], idx[keep][inside]], 1).astype(np.float64))
                        cand[-1] = np.concatenate([cand[-1], D[keep][inside][:, None]], 1)
            if cand:
                c = np.concatenate(cand)
                c = c[np.lexsort((c[:, 1], c[:, 2], c[:, 0]))]
                top = np.concatenate([[True], c[1:, 0] != c[:-1, 0]])[:-1]                    # the pixel's winner and its runner-up
                same = top & (c[1:, 0] == c[:-1, 0]) & (c[1:, 2] - c[:-1, 2] < m['dpair'])
                for a, b in zip(c[:-1][same, 1].astype(int), c[1:][same, 1].astype(int)):
                    if a != b and xyz[a].tobytes() != xyz[b].tobytes():
                        bad_pt.add(int(b))
            for k, b in enumerate(self.boxes):
                if b['view'] != vi or not np.isfinite(corners[b['box']]).all():
                    continue
                X, Y, D, W = FR.project(v['P'], corners[b['box']])
                if (np.abs(W - v['w_near']) < m['w']).any():
                    bad_box.add(k)
                for e in FR.box_edges(v['P'], v['w_near'], corners[b['box']]):
                    if e is not None and any(abs(t) < FR.PIX_CLAMP and on_edge(t + 0.5, m['seg']) for t in e):
                        bad_box.add(k)
            for k, r in enumerate(self.rects):
                if r['view'] == vi and any(np.isfinite(r[key]) and on_edge(float(np.float32(r[key])) + 0.5, m['rect']) for key in ('xmin', 'ymin', 'xmax', 'ymax')):
                    bad_rect.add(k)
        return bad_pt, bad_box, bad_rect

    def repair(self):
        for _ in range(50):
            pts, boxes, rects = self.bad_primitives()
            if not (pts or boxes or rects):
                break
            for i in sorted(pts):
                assert self.draw_pt[i] is not None, '%s: hand-built point %d sits inside a margin' % (self.name, i)
                self.xyz[i], self.rgb[i] = np.asarray(self.draw_pt[i](self.r), np.float64), self.r.uniform(0, 1, 3)
            for k in sorted(boxes):
                j = self.boxes[k]['box']
                assert self.draw_box[j] is not None, '%s: hand-built box %d sits inside a margin' % (self.name, k)
                self.corners[j] = np.asarray(self.draw_box[j](self.r), np.float64).reshape(8, 3)
            for k in sorted(rects):
                assert self.draw_rect[k] is not None, '%s: hand-built rectangle %d sits inside a margin' % (self.name, k)
                self.rects[k].update(self.draw_rect[k](self.r))
            self.redrawn += len(pts) + len(boxes) + len(rects)
        else:
            raise AssertionError('%s: the repair does not settle' % self.name)
        assert self.redrawn <= MAX_REDRAWN * self.n_primitives, '%s: %d of %d primitives redrawn' % (self.name, self.redrawn, self.n_primitives)
        return self


def box_corners(centre, size, ry):
    """get_3d_box order in upright camera coordinates: rows 0-3 the +h/2 face (fake_detect.get_3d_box)."""
    import fake_detect as FD
    l, w, h = size
    return FD.get_3d_box(l, w, h, ry, tuple(centre))


# the segments of the issue's list, as (a, b) pixel pairs of the 64 x 48 view; quarter-pixel coordinates keep clear of every rounding boundary
SEGMENTS_A = [((2.25, 3.25), (7.25, 3.25)),         # horizontal
              ((10.25, 5.25), (10.25, 30.25)),      # vertical
              ((15.25, 5.25), (35.25, 25.25)),      # diagonal, down
              ((15.25, 40.25), (40.25, 15.25)),     # diagonal, up
              ((50.25, 40.25), (50.25, 40.25)),     # zero length
              ((40.25, 2.25), (60.25, 12.25))]      # the 2 : 1 slope
SEGMENTS_B = [((3.25, 4.25), (44.25, 15.25)),       # shallow, down
              ((3.25, 30.25), (47.25, 18.25)),      # shallow, up
              ((50.25, 3.25), (57.25, 44.25)),      # steep, down
              ((30.25, 44.25), (36.25, 20.25)),     # steep, up
              ((5.25, 40.25), (6.25, 46.25)),       # steep and short
              ((20.25, 36.25), (29.25, 37.25))]     # one step of the minor axis half-way
FAR = [((30.25, 20.25), (-500.75, 35.25)), ((30.25, 22.25), (600.25, 10.25)), ((25.25, 20.25), (33.25, -400.75)),
       ((40.25, 25.25), (28.25, 700.25)), ((-300.75, -200.75), (400.25, 300.25)), ((-50.75, 10.25), (-3.75, 60.25))]


def segment_case(name, segments, reverse=False, thickness=1):
    c = Case(name)
    for k, (a, b) in enumerate(segments):
        a, b = (b, a) if reverse else (a, b)
        c.add_segment(0, a, b, colour_of(k), thickness)
        c.add_segment(1, (a[0] * 0.5, a[1] * 0.375 - 0.125), (b[0] * 0.5, b[1] * 0.375 - 0.125), colour_of(k + 7), thickness)
    return c.repair()


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case (repaired; built once per process and shared by the tests: nothing changes them)."""
    out = {}

    # two overlapping planes of points at different depths, seen by both views (the second through a scaled matrix)
    c = Case('planes', seed=1, P=(ORTHO, ortho(0.5, 0.35, 0.3, -0.2)))
    lo = lambda r: np.array([r.uniform(-2, 66), r.uniform(-2, 50), 2.0 + 0.01 * r.uniform(-1, 1)])
    hi = lambda r: np.array([r.uniform(20, 50), r.uniform(10, 40), 1.0 + 0.5 * r.uniform(0, 1)])
    c.add_points(0, [lo(c.r) for _ in range(1000)], lo, FR.RGB)
    c.add_points(0, [hi(c.r) for _ in range(800)], hi, FR.LABEL, colour_of(3), colour_of(4))
    c.add_range(1, 0, 1000, FR.FLAT, colour_of(5))
    c.add_range(1, 1000, 800, FR.RGB, splat=3)
    out[c.name] = c.repair()

    # an exact tie in D, hand-built with equal coordinates: the lower index wins, in whichever range it lies
    c = Case('tie')
    c.add_points(0, [(5.25, 5.25, 2.0), (9.25, 9.25, 3.0)], None, FR.FLAT, colour_of(1))
    c.add_points(0, [(5.25, 5.25, 2.0), (9.25, 9.25, 3.0), (5.25, 5.25, 2.0)], None, FR.FLAT, colour_of(2), splat=3)
    c.add_range(1, 2, 3, FR.FLAT, colour_of(3), splat=5)
    c.add_range(1, 0, 2, FR.FLAT, colour_of(4), splat=5)
    out[c.name] = c.repair()

    # splat 1, 3 and 5 at the four borders and corners, and just outside them
    c = Case('splat')
    for k, s in enumerate((1, 3, 5)):
        for vi, (H, W) in enumerate(SIZES):
            spots = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (0, H // 2), (W - 1, H // 2), (W // 2, H - 1),
                     (-1, H // 3), (W, H // 3), (W // 3, -2), (W // 3, H + 1), (-2, -2), (W + 1, H + 1), (-3, 3), (W // 4, H // 4)]
            c.add_points(vi, [(x + 0.25 - 0.125 * k, y - 0.25 + 0.125 * k, 1.0 + k + 0.03125 * j) for j, (x, y) in enumerate(spots)], None, FR.FLAT, colour_of(k + 3 * vi), splat=s)
    out[c.name] = c.repair()

    out['segments_a'] = segment_case('segments_a', SEGMENTS_A)
    out['segments_a_reversed'] = segment_case('segments_a_reversed', SEGMENTS_A, reverse=True)
    out['segments_b'] = segment_case('segments_b', SEGMENTS_B)
    out['segments_b_reversed'] = segment_case('segments_b_reversed', SEGMENTS_B, reverse=True)
    out['far_endpoints'] = segment_case('far_endpoints', FAR)
    out['far_endpoints_thick'] = segment_case('far_endpoints_thick', FAR, reverse=True, thickness=4)

    # thickness 1, 2, 3 and 5 along the four borders, and rectangles on them
    c = Case('thickness')
    for vi, (H, W) in enumerate(SIZES):
        c.add_segment(vi, (0.25, 0.25), (W - 0.75, 0.25), colour_of(1), 2)
        c.add_segment(vi, (0.25, 0.25), (0.25, H - 0.75), colour_of(2), 3)
        c.add_segment(vi, (W - 0.75, 1.25), (W - 0.75, H - 0.75), colour_of(3), 5)
        c.add_rect(vi, -0.75, H - 1.25, W + 3.25, H - 1.25, colour_of(4), 1)
        c.add_rect(vi, 0.25, 0.25, W - 0.75, H - 0.75, colour_of(5), 2)
        c.add_rect(vi, W - 3.75, H - 4.75, W + 1.25, H + 2.25, colour_of(6), 5)
    out[c.name] = c.repair()

    # a pinhole view: a box crossing the near plane, a box wholly behind it (paints nothing), a box with a NaN corner, boxes in front
    c = Case('near_plane', seed=3, P=(pinhole(40.0, 32.0, 24.0), pinhole(20.0, 16.0, 8.0)), w_near=(0.5, 0.75))
    pt = lambda r: np.array([r.uniform(-3, 3), r.uniform(-2, 2), r.uniform(-1, 6) if r.uniform() < 0.2 else r.uniform(1, 6)])
    c.add_points(0, [pt(c.r) for _ in range(600)], pt, FR.RGB)
    c.add_range(1, 0, 600, FR.LABEL, colour_of(1), colour_of(2), splat=3)
    crossing = lambda r: box_corners((r.uniform(-0.5, 0.5), r.uniform(-0.3, 0.3), r.uniform(0.9, 1.1)), (1.5, 0.8, 0.6), r.uniform(0.2, 1.2))
    behind = lambda r: box_corners((0.2, 0.1, -2.0), (1.0, 1.0, 1.0), r.uniform(0, 1))
    front = lambda r: box_corners((r.uniform(-1.5, 1.5), r.uniform(-0.5, 0.5), r.uniform(3, 5)), r.uniform(0.5, 1.5, 3), r.uniform(-3, 3))
    for vi in range(2):
        c.add_box(vi, crossing(c.r), colour_of(3), 1 + vi, crossing)
        c.add_box(vi, behind(c.r), colour_of(4), 1, behind)
        nan = front(c.r)
        nan[5, 1] = np.nan
        c.add_box(vi, nan, colour_of(5), 2)
    c.add_box(0, front(c.r), colour_of(6), 1, front)
    c.add_box(1, front(c.r), colour_of(7), 3, front)
    out[c.name] = c.repair()

    # painting order: box over points, later box over earlier, rectangle over box
    c = Case('order', seed=4)
    pt = lambda r: np.array([r.uniform(5, 60), r.uniform(5, 44), r.uniform(1, 2)])
    c.add_points(0, [pt(c.r) for _ in range(1500)], pt, FR.FLAT, colour_of(1), splat=3)
    c.add_range(1, 0, 1500, FR.RGB, splat=1)
    for vi, s in ((0, 1.0), (1, 0.375)):
        c.add_segment(vi, (8.25 * s, 8.25 * s), (55.25 * s, 35.25 * s), colour_of(2), 3)
        c.add_segment(vi, (8.25 * s, 35.25 * s), (55.25 * s, 8.25 * s), colour_of(3), 3)      # crosses the first: it is on top
        c.add_segment(vi, (30.25 * s, 2.25 * s), (30.25 * s, 40.25 * s), colour_of(4), 1)
        c.add_rect(vi, 20.25 * s, 10.25 * s, 45.25 * s, 30.25 * s, colour_of(5), 2)             # over all boxes
        c.add_rect(vi, 25.25 * s, 10.25 * s, 50.25 * s, 36.25 * s, colour_of(6), 1)             # and over the first rectangle
    out[c.name] = c.repair()

    # a background image under the first view, a colour under the second, which has no primitives at all
    r = np.random.RandomState(5)
    c = Case('background', seed=5, images=(r.randint(0, 256, (SIZES[0][0], SIZES[0][1], 3)).astype(np.uint8), None),
             bg_colours=((0.0, 0.0, 0.0), (200 / 255.0, 100 / 255.0, 1.0)))
    pt = lambda r: np.array([r.uniform(0, 64), r.uniform(0, 48), r.uniform(1, 2)])
    c.add_points(0, [pt(c.r) for _ in range(200)], pt, FR.LABEL, colour_of(1), colour_of(2))
    c.add_segment(0, (3.25, 40.25), (60.25, 44.25), colour_of(3), 2)
    out[c.name] = c.repair()

    # both backgrounds from images, everything at once, at random
    r = np.random.RandomState(6)
    c = Case('random', seed=6, P=(pinhole(35.0, 30.0, 22.0), pinhole(18.0, 17.0, 9.0)), w_near=(0.5, 0.5),
             images=tuple(r.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES))
    pt = lambda r: np.array([r.uniform(-4, 4), r.uniform(-3, 3), r.uniform(1, 6)])
    c.add_points(0, [pt(c.r) for _ in range(2000)], pt, FR.RGB, splat=3)
    c.add_range(1, 500, 1500, FR.LABEL, colour_of(1), colour_of(2), splat=5)
    for k in range(3):
        c.add_box(0, front(c.r), colour_of(3 + k), 1 + k, front)
        c.add_box(1, front(c.r), colour_of(6 + k), 1 + k % 2, front)
    rect = lambda r: dict(xmin=r.uniform(-5, 30), ymin=r.uniform(-5, 20), xmax=r.uniform(31, 70), ymax=r.uniform(21, 55))
    for k in range(3):
        c.add_rect(k % 2, colour=colour_of(9 + k), thickness=1 + k, draw=rect, **rect(c.r))
    out[c.name] = c.repair()
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    want = cases()[name].expected()
    want.setflags(write=False)
    return want


def tables_of(case):
    """The ctypes tables of a case -> (views, ranges, boxes, rects) as (table, n) pairs, total pixels, bytes of out, the background bytes."""
    offs, n_out, bg_offs, bg = case.layout()
    col = lambda c: (C.c_float * 3)(*[float(x) for x in c])
    views, px = [], 0
    for i, v in enumerate(case.views):
        views.append(abi.RenderView((C.c_float * 16)(*v['P'].reshape(16).tolist()), v['w_near'], v['H'], v['W'], px, offs[i], bg_offs[i], col(v['bg_colour']), 0))
        px += v['H'] * v['W']
    ranges, pos = [], 0
    for r in case.ranges:
        ranges.append(abi.RenderPoints(r['view'], r['first'], r['count'], r['mode'], col(r['colour0']), col(r['colour1']), r['splat'], 0, pos))
        pos += r['count']
    boxes = [abi.RenderBox(b['view'], b['box'], col(b['colour']), b['thickness']) for b in case.boxes]
    rects = [abi.RenderRect(r['view'], r['xmin'], r['ymin'], r['xmax'], r['ymax'], col(r['colour']), r['thickness']) for r in case.rects]
    t = lambda cls, rows: (R._table(cls, rows), len(rows))
    return t(abi.RenderView, views), t(abi.RenderPoints, ranges), t(abi.RenderBox, boxes), t(abi.RenderRect, rects), px, n_out, bg


def run_case(rt, case, renderer=None, mirrors=True):
    """The case through render.Renderer.render_tables on `rt` -> the whole `out` buffer as a NumPy array."""
    ren = renderer or R.Renderer(rt)
    views, ranges, boxes, rects, px, n_out, bg = tables_of(case)
    xyz, rgb, label, corners = case.arrays()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device) if a is not None and a.size else None
    out = torch.from_numpy(fill_pattern(n_out)).to(rt.device)
    ren.render_tables(views, up(xyz), up(rgb), up(label), ranges, up(corners), boxes, rects, out, bg=up(bg), mirrors=mirrors)
    return out.cpu().numpy().copy()


def assert_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.nonzero(got != want)[0]
    assert not len(diff), (what, '%d bytes differ' % len(diff), diff[:8], got[diff[:8]], want[diff[:8]])


def view_image(case, buf, i):
    offs, _, _, _ = case.layout()
    v = case.views[i]
    return buf[offs[i]:offs[i] + 3 * v['H'] * v['W']].reshape(v['H'], v['W'], 3)


# ---- the fixture scenes ------------------------------------------------------------------------------------------------------------------
SCENE_SIZE = (240, 320)


@functools.lru_cache(maxsize=None)
def scenes():
    """The three scenes of tests/golden/frustum_scenes.npz -> [{'id', 'xyz' (upright camera), 'rgb', 'Rtilt', 'K', 'image' (RGB), 'gt' [g,8,3],
    'gt_classes', 'dets' [(class, box2d, prob)]}] and the reference's projections of render_reference.npz."""
    import tempfile
    import frustum_check as FC
    from transferable3d_amd import sunrgbd_data as SD
    root = tempfile.mkdtemp()
    ids, det, _ = FC.write_golden_scenes(root)
    ds = SD.sunrgbd_object(root)
    det_id, det_type, det_box, det_prob = SD.read_det_folder(det)
    out = []
    for s in ids:
        depth, calib, objs = ds.get_depth(s), ds.get_calibration(s), ds.get_label_objects(s)
        out.append(dict(id=s, depth=depth, xyz=SD.flip_axis_to_camera(depth[:, :3]), rgb=depth[:, 3:6], Rtilt=calib.Rtilt, K=calib.K,
                        image=np.ascontiguousarray(ds.get_image(s)[:, :, ::-1]), gt=np.stack([SD.compute_box_3d(o) for o in objs]),
                        gt_classes=[o.classname for o in objs],
                        dets=[(t, b, p) for i, t, b, p in zip(det_id, det_type, det_box, det_prob) if i == s]))
    return out, np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'render_reference.npz'))


@functools.lru_cache(maxsize=None)
def scene_case(k):
    """Scene k at 320 x 240: the camera view with the image, the points in their colours, the label boxes (thickness 3, one colour per
    box) and the detection rectangles.  A point or box inside a margin is redrawn two millimetres (a fifth of a pixel) away."""
    sc = scenes()[0][k]
    cam = R.image_view(sc['Rtilt'], sc['K'], *SCENE_SIZE, image=sc['image'])
    c = Case('scene_%d' % sc['id'], seed=50 + k, P=(cam.P,), w_near=(cam.w_near,), images=(sc['image'],), sizes=(SCENE_SIZE,))
    jitter = lambda p: (lambda r: p + r.normal(0, 2e-3, p.shape))
    first = len(c.xyz)
    for p, col in zip(sc['xyz'], sc['rgb']):
        c.xyz.append(p)
        c.rgb.append(col)
        c.label.append(0)
        c.draw_pt.append(jitter(p))
    c.add_range(0, first, len(sc['xyz']), FR.RGB)
    for j, k8 in enumerate(sc['gt']):
        c.add_box(0, k8, colour_of(j), 3, jitter(k8))
    for j, (_, b, _) in enumerate(sc['dets']):
        c.add_rect(0, b[0], b[1], b[2], b[3], colour_of(8 + j), 1, lambda r, b=b: dict(zip(('xmin', 'ymin', 'xmax', 'ymax'), b + r.normal(0, 0.01, 4))))
    return c.repair()


def later_owner(case, view, box_entry):
    """[H,W] bool: the pixels of `view` that a primitive later in the painting order than box entry `box_entry` paints."""
    v = case.views[view]
    _, _, _, corners = case.arrays()
    o = np.zeros((v['H'], v['W']), np.int64)
    for k, b in enumerate(case.boxes):
        if b['view'] == view and k > box_entry:
            for e in FR.box_edges(v['P'], v['w_near'], corners[b['box']]):
                FR.stamp(o, e, b['thickness'], 1, v['H'], v['W'])
    for r in case.rects:
        if r['view'] == view:
            for e in FR.rect_edges(r['xmin'], r['ymin'], r['xmax'], r['ymax']):
                FR.stamp(o, e, r['thickness'], 1, v['H'], v['W'])
    return o > 0


def check_reference_corners(case, k, buf):
    """Every reference box3d_pts_2d corner inside the image carries its box's colour in the camera view of `buf`, unless a primitive
    later in the painting order lies over it.  -> (corners checked, corners painted over)."""
    sc, ref = scenes()[0][k], scenes()[1]
    img = view_image(case, buf, 0)
    H, W = SCENE_SIZE
    uv = ref['box_uv_%d' % sc['id']]
    checked = covered = 0
    for j in range(len(uv)):
        entry = [e for e, b in enumerate(case.boxes) if b['view'] == 0][j]
        later = later_owner(case, 0, entry)
        want = tuple(FR.to_byte(case.boxes[entry]['colour']).tolist())
        for u, v in uv[j]:
            px, py = int(np.floor(u + 0.5)), int(np.floor(v + 0.5))
            if 0 <= px < W and 0 <= py < H:
                checked += 1
                if later[py, px]:
                    covered += 1
                else:
                    assert tuple(img[py, px].tolist()) == want, (case.name, j, (px, py), img[py, px], want)
    return checked, covered


# ---- error cases -----------------------------------------------------------------------------------------------------------------------
def error_calls(rt):
    """[(what, expected return code, callable -> return code)]: every error the header names, on a small valid call with one thing wrong.
    Nothing is launched by any of them (the checks come first), so they run on either library."""
    c = cases()['order']
    views, ranges, boxes, rects, px, n_out, bg = tables_of(c)
    xyz, rgb, label, corners = c.arrays()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)
    held = dict(xyz=up(xyz), rgb=up(rgb), label=up(label), corners=up(corners), out=torch.zeros(n_out, dtype=torch.uint8, device=rt.device),
                ws=torch.zeros(px * 12 // 8 + 2, dtype=torch.int64, device=rt.device))
    dev = {k: torch.from_numpy(R._bytes_of(t, n)).to(rt.device) for k, (t, n) in dict(views=views, ranges=ranges, boxes=boxes, rects=rects).items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def args(**change):
        a = abi.RenderArgs(2, len(xyz), ranges[1], len(corners), boxes[1], rects[1], 3, ptr(dev['views']), abi.fptr(held['xyz']),
                           abi.fptr(held['rgb']), abi.u8ptr(held['label']), ptr(dev['ranges']), abi.fptr(held['corners']), ptr(dev['boxes']),
                           ptr(dev['rects']), px, sum(r['count'] for r in c.ranges), abi.u8ptr(None), 0, abi.u8ptr(held['out']), n_out,
                           ptr(held['ws']), px * 12, C.cast(views[0], C.c_void_p), C.cast(ranges[0], C.c_void_p),
                           C.cast(boxes[0], C.c_void_p), C.cast(rects[0], C.c_void_p))
        for k, v in change.items():
            setattr(a, k, v)
        return a

    def with_entry(table, cls, n, i, mirror, **change):
        """A copy of a host table with entry i changed, as the mirror of that table."""
        t = (cls * n)()
        C.memmove(t, table, n * C.sizeof(cls))
        for k, v in change.items():
            setattr(t[i], k, v)
        held.setdefault('tables', []).append(t)
        return args(**{mirror: C.cast(t, C.c_void_p)})

    call = lambda a: rt.lib.t3d_render(C.byref(a), rt.stream())
    null = C.c_void_p(0)
    out = [('a null args pointer', -1, lambda: rt.lib.t3d_render(C.cast(null, C.POINTER(abi.RenderArgs)), rt.stream())) if not isinstance(rt.lib, FR.RenderSpec)
           else ('no views, nothing else: T3D_OK', 0, lambda: call(abi.RenderArgs()))]
    out += [('no views: T3D_OK whatever else is wrong', 0, lambda: call(args(n_views=0, out=abi.u8ptr(None)))),
            ('a null view table', -1, lambda: call(args(views=null))),
            ('a null out', -1, lambda: call(args(out=abi.u8ptr(None)))),
            ('a null workspace', -1, lambda: call(args(workspace=null))),
            ('a null point array with ranges', -1, lambda: call(args(xyz=abi.fptr(None)))),
            ('a null range table with ranges', -1, lambda: call(args(ranges=null))),
            ('a null corner array with boxes', -1, lambda: call(args(corners=abi.fptr(None)))),
            ('a null box table with boxes', -1, lambda: call(args(boxes=null))),
            ('a null rectangle table with rectangles', -1, lambda: call(args(rects=null))),
            ('a negative view count', -1, lambda: call(args(n_views=-1))),
            ('a negative point count', -1, lambda: call(args(n_points=-1))),
            ('a negative range count', -1, lambda: call(args(n_ranges=-1))),
            ('a negative box count', -1, lambda: call(args(n_boxes=-2))),
            ('a negative rectangle count', -1, lambda: call(args(n_rects=-1))),
            ('no pixels', -1, lambda: call(args(total_pixels=0))),
            ('a workspace one byte short', -1, lambda: call(args(workspace_bytes=px * 12 - 1))),
            ('a misaligned workspace', -1, lambda: call(args(workspace=C.c_void_p(held['ws'].data_ptr() + 4)))),
            ('H * W == 0', -1, lambda: call(with_entry(views[0], abi.RenderView, 2, 1, 'views_host', H=0))),
            ('a range naming a view >= V', -1, lambda: call(with_entry(ranges[0], abi.RenderPoints, ranges[1], 0, 'ranges_host', view=2))),
            ('a box naming a view >= V', -1, lambda: call(with_entry(boxes[0], abi.RenderBox, boxes[1], 1, 'boxes_host', view=7))),
            ('a rectangle naming a view >= V', -1, lambda: call(with_entry(rects[0], abi.RenderRect, rects[1], 0, 'rects_host', view=2))),
            ('a splat of 2', -1, lambda: call(with_entry(ranges[0], abi.RenderPoints, ranges[1], 1, 'ranges_host', splat=2))),
            ('a splat of 7', -1, lambda: call(with_entry(ranges[0], abi.RenderPoints, ranges[1], 1, 'ranges_host', splat=7))),
            ('a thickness of 0', -1, lambda: call(with_entry(boxes[0], abi.RenderBox, boxes[1], 0, 'boxes_host', thickness=0))),
            ('a thickness of 6', -1, lambda: call(with_entry(rects[0], abi.RenderRect, rects[1], 1, 'rects_host', thickness=6))),
            ('a box index past the corners', -1, lambda: call(with_entry(boxes[0], abi.RenderBox, boxes[1], 0, 'boxes_host', box=len(corners)))),
            ('a range past the points', -1, lambda: call(with_entry(ranges[0], abi.RenderPoints, ranges[1], 0, 'ranges_host', first=1))),
            ('an image past the end of out', -1, lambda: call(with_entry(views[0], abi.RenderView, 2, 1, 'views_host', out_offset=n_out - 8))),
            ('a background without a bg buffer', -1, lambda: call(with_entry(views[0], abi.RenderView, 2, 0, 'views_host', bg_offset=0))),
            ('a struct of another size', abi.ERR_ABI, lambda: call(args(struct_size=C.sizeof(abi.RenderArgs) - 8)))]
    return out


# ---- the viewer ------------------------------------------------------------------------------------------------------------------------
def synthetic_prediction_files(root, n=14, N=192, seed=7):
    """A ground-truth frustum file of `n` synthetic frustums (two per image; every other label box stored bottom face first) and two
    prediction files of them in test_semisup's 14-list layout: `with_points` holds the network's points (centre view) and both masks,
    `file_run` holds neither (what test_semisup writes for a frustum file).  The predictions are the labels with noise.
    -> (gt path, [with_points path, file_run path], the 14-list)."""
    import os
    from transferable3d_amd import viewer as VW
    from transferable3d_amd.constants import MEAN_DIMS_ARR, NUM_HEADING_BIN, class2type
    from transferable3d_amd.dataset import save_zipped_pickle, synthetic_frustums
    from transferable3d_amd.eval_det import get_3d_box
    r = np.random.RandomState(seed)
    f = synthetic_frustums(n, num_channel=6, seed=seed, min_points=300, max_points=600)
    cls = np.arange(n) % 4                                        # four classes, so that the choice has shares to split
    size = MEAN_DIMS_ARR[cls] + r.normal(0, 0.05, (n, 3))
    gt = [[] for _ in range(13)]
    p = [[] for _ in range(14)]
    for i in range(n):
        pts, seg = f['points'][f['offsets'][i]:f['offsets'][i + 1]], f['seg'][f['offsets'][i]:f['offsets'][i + 1]]
        k = get_3d_box(size[i], f['heading'][i], f['box_center'][i])
        stored = k if i % 2 == 0 else k[[4, 5, 6, 7, 0, 1, 2, 3]]
        for lst, v in zip(gt, (100 + i // 2, np.array([10.0, 10.0, 60.0, 60.0]), stored, None, pts.astype(np.float64), seg.astype(np.float64),
                               class2type[int(cls[i])], f['heading'][i], size[i], np.eye(3), np.eye(3), f['frustum_angle'][i], [530, 730])):
            lst.append(v)
        rot = np.pi / 2 + f['frustum_angle'][i]
        sel = r.choice(len(pts), N, replace=len(pts) < N)
        seg_pred = seg[sel].copy()
        flip = r.uniform(size=N) < 0.15
        seg_pred[flip] = 1 - seg_pred[flip]
        heading = (f['heading'][i] - rot + r.normal(0, 0.1)) % (2 * np.pi)
        hcls = int(np.round(heading / (2 * np.pi / NUM_HEADING_BIN))) % NUM_HEADING_BIN
        hres = heading - hcls * (2 * np.pi / NUM_HEADING_BIN)
        hres = hres - 2 * np.pi if hres > np.pi else hres
        centre = VW.rotate_along_y(f['box_center'][i][None], rot)[0] + r.normal(0, 0.08, 3)
        for lst, v in zip(p, (np.concatenate([VW.rotate_along_y(pts[sel, :3], rot), pts[sel, 3:]], 1).astype(np.float32), seg[sel].astype(np.int64),
                              seg_pred.astype(np.int64), centre, hcls, hres, int(cls[i]), size[i] - MEAN_DIMS_ARR[cls[i]] + r.normal(0, 0.05, 3),
                              rot, float(r.uniform(0, 1)), int(cls[i]), 100 + i // 2, None, stored)):
            lst.append(v)
    p[12] = None
    gt_path = os.path.join(str(root), 'gt_frustums.zip.pickle')
    save_zipped_pickle(gt, gt_path)
    with_points, file_run = os.path.join(str(root), 'with_points.zip.pickle'), os.path.join(str(root), 'file_run.zip.pickle')
    save_zipped_pickle(p, with_points, protocol=4)
    save_zipped_pickle([None, None] + p[2:], file_run, protocol=4)
    return gt_path, [with_points, file_run], p


def check_viewer(rt, root, box_iou_bound):
    """python -m transferable3d_amd.viewer end to end on `rt`: --vis pred3d on the synthetic files above (the sheet, the legend, the
    `Mean Box IOU` / `Mean Seg IOU` lines against values computed here, the AP block), --vis fpc on a fixture scene with and without
    --rgb_detection, the message of the other modes.  box_iou_bound: how far the logged mean box IoU may lie from the fp64 value of
    fake_nms.iou_corners on the fp32-rounded corners.  -> report lines."""
    import json
    import os
    import re
    import pytest
    import fake_nms as FN
    import frustum_check as FC
    from transferable3d_amd import viewer as VW
    from transferable3d_amd.constants import class2type
    gt_path, pred_files, p = synthetic_prediction_files(root)
    n, out = len(p[3]), os.path.join(str(root), 'vis')
    logged = []
    res = VW.main(['--vis', 'pred3d', '--pred_files'] + pred_files + ['--gt_file', gt_path, '--num', '7', '--seed', '3', '--out_dir', out], rt=rt,
                  log=logged.append)
    # the values, computed here: the predicted box from the 14-list by the reference's formulas, the IoU in fp64
    pred = VW.predicted_boxes(p)
    iou64 = lambda i: FN.iou_corners(VW.y_max_face_first(p[13][i]).astype(np.float32), pred[i].astype(np.float32))[0]      # fp64 on the fp32 corners the entry point takes
    want_box = float(np.mean([iou64(i) for i in range(n)]))
    ious = []
    for i in range(n):
        g, q = np.asarray(p[1][i]) != 0, np.asarray(p[2][i]) != 0
        fg, bg = (g & q).sum() / float((g | q).sum()), (~g & ~q).sum() / float((~g | ~q).sum())
        ious.append(0.5 * (fg + bg))
    want_seg = float(np.mean(ious))
    assert 0.2 < want_box < 0.95 and 0.5 < want_seg < 0.95, (want_box, want_seg)      # noisy predictions: neither perfect nor useless
    box_lines = [float(re.search(r'Mean Box IOU: ([0-9.]+)', l).group(1)) for l in logged if 'Mean Box IOU' in l]
    seg_lines = [l for l in logged if 'Mean Seg IOU' in l]
    assert len(box_lines) == 2 and all(abs(v - want_box) <= box_iou_bound + 5e-7 for v in box_lines), (box_lines, want_box)       # (%f prints to 1e-6)
    assert len(seg_lines) == 2 and seg_lines[0] == 'Mean Seg IOU: %f' % want_seg and 'not available' in seg_lines[1], seg_lines
    assert abs(res[0]['mean_seg_iou'] - want_seg) < 1e-12 and res[1]['mean_seg_iou'] is None
    assert sum('Average Precision:' in l and 'Mean AP' in l for l in logged) == 2
    assert any(l == 'Number of objects in whitelist: 4' for l in logged)
    chosen = res[0]['chosen']
    assert len(chosen) == len(set(chosen)) == 7 and res[1]['chosen'] == chosen
    assert sorted(np.bincount([int(p[10][i]) for i in chosen], minlength=4).tolist()) == [1, 2, 2, 2]      # array_split's shares of 7 over 4 classes
    again = VW.choose(p[10], p[11], 7, 3)
    assert again == chosen and VW.choose(p[10], p[11], 7, 4) != chosen
    assert set(int(p[11][i]) for i in VW.choose(p[10], p[11], 7, 3, filenums={100, 101})) <= {100, 101}
    for k, name in enumerate(('with_points', 'file_run')):
        sheet = R.read_png(os.path.join(out, 'pred3d_%s.png' % name))
        legend = json.load(open(os.path.join(out, 'pred3d_%s.json' % name)))
        tile_h, tile_w = VW.TILE, 2 * VW.TILE + 2
        assert sheet.shape == (2 * tile_h + 4, 5 * tile_w + 4 * 4, 3) and legend['tile'] == [tile_h, tile_w]
        assert [t['prediction'] for t in legend['tiles']] == chosen and [t['class'] for t in legend['tiles']] == [class2type[int(p[10][i])] for i in chosen]
        assert abs(legend['mean_box_iou'] - want_box) <= box_iou_bound
        for j, t in enumerate(legend['tiles']):
            r_, c_ = divmod(j, 5)
            tile = sheet[r_ * (tile_h + 4):r_ * (tile_h + 4) + tile_h, c_ * (tile_w + 4):c_ * (tile_w + 4) + tile_w]
            for panel in (tile[:, :VW.TILE], tile[:, VW.TILE + 2:]):                      # both boxes and points in both panels
                has = lambda c: bool((panel == FR.to_byte(c)).all(2).any())
                assert has(R.GT_COLOUR) and has(R.PRED_COLOUR), (name, j)
                palette = R.MASK_AGREEMENT if k == 0 else R.MASK_COLOURS
                assert sum(has(c) for c in palette) >= 2, (name, j)
            assert abs(t['box_iou'] - iou64(t['prediction'])) <= box_iou_bound
            assert (t['seg_iou'] is None) == (k == 1) and (k == 1 or abs(t['seg_iou'] - ious[t['prediction']]) < 1e-12)
    report = ['pred3d: mean box IoU %.6f (fp64 %.6f), mean seg IoU %.6f, 7 tiles of classes %s' % (box_lines[0], want_box, want_seg, [t['class'] for t in legend['tiles']])]
    # fpc on a fixture scene
    ids, det, _ = FC.write_golden_scenes(root)
    scene = scenes()[0][0]
    for extra in ([], ['--rgb_detection', '--rgb_detection_path', det]):
        sub = os.path.join(out, 'fpc_det' if extra else 'fpc')
        path, legend = VW.main(['--vis', 'fpc', '--filenum', str(ids[0]), '--dataset_dir', str(root), '--out_dir', sub] + extra, rt=rt, log=logged.append)
        img = R.read_png(path)
        assert img.shape == scene['image'].shape and legend == json.load(open(os.path.join(sub, 'fpc_%06d.json' % ids[0])))['objects']
        whitelisted = [c for c in scene['gt_classes'] if c in ('bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub')]
        assert len(legend) >= 2 and (extra or [o['class'] for o in legend] == whitelisted)
        ys, xs = np.mgrid[0:img.shape[0], 0:img.shape[1]]
        for o in legend:
            mine = (img == FR.to_byte(o['colour'])).all(2)
            x0, y0, x1, y1 = o['box2d']
            inside = (xs >= x0 - 3) & (xs <= x1 + 3) & (ys >= y0 - 3) & (ys <= y1 + 3)      # a splat of 3 and a rectangle of thickness 2 around the box
            assert mine.sum() >= 20 and (mine & ~inside).sum() == 0, (o['class'], int(mine.sum()), int((mine & ~inside).sum()))
        assert 0.02 < (img != scene['image']).any(2).mean() < 0.9
        report.append('fpc%s: %d frustums, %d pixels painted' % (' --rgb_detection' if extra else '', len(legend), int((img != scene['image']).any(2).sum())))
    for mode in ('pc', 'seg_box', 'box_pc', 'pred2d'):
        with pytest.raises(SystemExit, match='pred3d and fpc'):
            VW.main(['--vis', mode, '--filenum', '3', '--filename', 'x'], rt=rt, log=logged.append)
    for bad in (['--vis', 'pred3d'], ['--vis', 'pred3d', '--pred_files', pred_files[0]], ['--vis', 'fpc'], ['--vis', 'nothing']):
        with pytest.raises(SystemExit):
            VW.main(bad, rt=rt, log=logged.append)
    return report
