"""Learnable SUN-RGBD-format scenes from a seed: rooms of furniture made of oriented boxes, seen by a depth camera through ray casting
on the device (csrc/scene_synth.hip, t3d_scene_raycast), with 3-D labels and the output of a simulated 2-D detector.

    python -m transferable3d_amd.synth_scenes --out D --scenes 200 --seed 1                  # D/training/..., D/det/, D/synth.json
    python -m transferable3d_amd.synth_scenes --out D --scenes 200 --frustum_dir F --no_files  # only the five frustum files of sunrgbd_data

What is modelled: a box room, a camera of a drawn height and tilt, 3 to --max_objects objects of the ten classes standing on the floor
along the walls (chairs preferably in rows at a table or desk), each made of a few boxes that tell its front from its back (a chair is a
seat, a back and four legs; the floor shows between them), occlusion, a depth noise growing with the square of the depth, dropped
pixels, a range limit and a grazing-angle limit; labels in the format SUNObject3d reads, with the 2-D box of the projected 3-D corners;
detections that miss, jitter, duplicate, confuse classes and fire on the background, in the format read_det_folder reads.
What is not: texture (every face is its part's colour times a shade), clutter beyond boxes, the holes a real sensor leaves at depth
edges, people, anything hanging on a wall.

The layout and the detector are host work on np.random.RandomState streams keyed by (seed, scene id); the pixels are the device's.  A
scene is a function of (seed, scene id, flags) alone, never of the batch it is cast in.
"""
import argparse
import collections
import ctypes as C
import io
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import abi
from . import sunrgbd_data as SD
from .constants import type_mean_size
from .dataset import save_zipped_pickle

PART_DTYPE = np.dtype([('centre', '<f8', 3), ('half', '<f8', 3), ('cos_r', '<f8'), ('sin_r', '<f8'), ('colour', '<f8', 3),
                       ('owner', '<i4'), ('reserved', '<i4')])
assert PART_DTYPE.itemsize == C.sizeof(abi.ScenePart)
CLASSES = SD.TYPE_WHITELIST
LABEL_LINE = '%s %.2f %.2f %.2f %.2f %f %f %f %f %f %f %f %f %f %f %f %f'

# Parts per class: (centre, half) as fractions of the label box's half sizes, in the object's frame (x: its front, the extent l; y: the
# extent w; z: up).  Every class but the table has a front.
_LEGS = lambda x0, x1, y, hx, hy, top: [((x, s * y, (top - 1.0) / 2.0), (hx, hy, (top + 1.0) / 2.0)) for x in (x0, x1) for s in (-1, 1)]
SHAPES = {
    'chair': [((0.1, 0, -0.05), (0.9, 1, 0.07)), ((-0.9, 0, 0.5), (0.1, 1, 0.5))] + _LEGS(-0.8, 0.85, 0.85, 0.1, 0.1, -0.12),
    'table': [((0, 0, 0.9), (1, 1, 0.1))] + _LEGS(-0.85, 0.85, 0.9, 0.08, 0.06, 0.8),
    'desk': [((0, 0, 0.9), (1, 1, 0.1)), ((-0.9, 0, 0.2), (0.04, 0.85, 0.55))] + _LEGS(-0.85, 0.85, 0.9, 0.08, 0.06, 0.8),
    'bed': [((0.05, 0, -0.3), (0.95, 1, 0.7)), ((-0.95, 0, 0), (0.05, 1, 1))],
    'sofa': [((0.15, 0, -0.45), (0.85, 0.8, 0.55)), ((-0.8, 0, 0), (0.2, 1, 1)), ((0.2, -0.9, -0.2), (0.8, 0.1, 0.8)),
             ((0.2, 0.9, -0.2), (0.8, 0.1, 0.8))],
    'toilet': [((0.3, 0, -0.5), (0.7, 0.8, 0.5)), ((-0.7, 0, 0), (0.3, 1, 1))],
    'bathtub': [((0, 0, -0.8), (1, 1, 0.2)), ((0, -0.9, 0.1), (1, 0.1, 0.9)), ((0, 0.9, 0.1), (1, 0.1, 0.9)),
                ((-0.9, 0, 0.1), (0.1, 0.8, 0.9)), ((0.9, 0, -0.1), (0.1, 0.8, 0.7))],
    'dresser': [((-0.05, 0, 0), (0.95, 1, 1)), ((0.96, 0, 0.5), (0.04, 0.9, 0.2)), ((0.96, 0, -0.3), (0.04, 0.9, 0.2))],
    'night_stand': [((-0.05, 0, 0.1), (0.95, 1, 0.9)), ((0.96, 0, 0.4), (0.04, 0.85, 0.3)), ((0, 0, -0.9), (0.8, 0.8, 0.1))],
    'bookshelf': [((-0.9, 0, 0), (0.1, 1, 1)), ((0.05, -0.95, 0), (0.85, 0.05, 1)), ((0.05, 0.95, 0), (0.85, 0.05, 1))] +
                 [((0.05, 0, z), (0.85, 0.9, 0.03)) for z in (-0.97, -0.35, 0.3, 0.97)],
}
COLOURS = {'bed': (170, 120, 160), 'table': (150, 110, 70), 'sofa': (90, 110, 160), 'chair': (120, 90, 60), 'toilet': (235, 235, 240),
           'desk': (130, 100, 80), 'dresser': (110, 80, 60), 'night_stand': (140, 105, 85), 'bookshelf': (100, 75, 55),
           'bathtub': (225, 230, 235)}
LOOK_ALIKE = {'table': 'desk', 'desk': 'table', 'sofa': 'bed', 'bed': 'sofa', 'night_stand': 'dresser', 'dresser': 'night_stand',
              'chair': 'toilet', 'toilet': 'chair', 'bookshelf': 'dresser', 'bathtub': 'bed'}

DEFAULTS = collections.OrderedDict(
    width=730, height=530, stride=1, max_objects=12, surface_inset=0.02, min_visible=20, noise_a=0.0015, p_drop=0.02, max_range=8.0,
    min_cos=0.17, det_miss=0.1, det_miss_occluded=3.0, det_full_visible=0.01, det_jitter=0.05, det_conf_a=6.0, det_conf_b=1.5, det_dup=0.15,
    det_dup_shift=0.15, det_confuse=0.05, det_fp_per_image=0.5, det_from_labels=False)


def _stream(seed, sid, purpose):
    return np.random.RandomState(np.array([seed & 0xFFFFFFFF, sid & 0xFFFFFFFF, purpose], np.uint32))


# ---- the device call ---------------------------------------------------------------------------------------------------------------------
class SceneCaster:
    """t3d_scene_raycast over a batch of scenes: one launch sequence, one copy back."""

    def __init__(self, rt, H, W, stride=1, seed=0, noise_a=0.0, p_drop=0.0, max_range=8.0, min_cos2=0.0):
        self.rt, self.H, self.W, self.stride, self.seed = rt, int(H), int(W), int(stride), int(seed)
        self.noise_a, self.p_drop, self.max_range, self.min_cos2 = float(noise_a), float(p_drop), float(max_range), float(min_cos2)
        self.last_kernel_ms = None

    def run(self, scenes, timed=False, on_device=False):
        """scenes: [{'id', 'Rtilt' (3,3), 'K' (3,3), 'room' (6,), 'parts' (PART_DTYPE array), 'n_objects'}].  Returns host arrays
        {'hit' [S,H,W], 'image' [S,H,W,3], 'points' [n,6], 'point_pixel' [n], 'scene_offsets' [S+1], 'visible' [S,64], 'vis_box' [S,64,4]}
        (on_device=True: the device tensors, points and point_pixel at their capacity, nothing copied back)."""
        dev, S, H, W = self.rt.device, len(scenes), self.H, self.W
        f64 = lambda k, n: np.ascontiguousarray(np.stack([np.asarray(s[k], np.float64).reshape(n) for s in scenes]))
        rtilt, K, room = f64('Rtilt', 9), f64('K', 9), f64('room', 6)
        sid = np.array([s['id'] for s in scenes], np.int64).astype(np.int32)
        counts = [len(s['parts']) for s in scenes]
        part_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        n_objects = np.array([s['n_objects'] for s in scenes], np.int32)
        parts = np.concatenate([np.asarray(s['parts'], PART_DTYPE) for s in scenes]) if S else np.zeros(0, PART_DTYPE)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        parts_t = up(parts.view(np.uint8).reshape(-1)) if len(parts) else None
        t = dict(rtilt=up(rtilt), K=up(K), scene_id=up(sid), room=up(room), part_offsets=up(part_offsets))
        hs, ws = -(-H // self.stride), -(-W // self.stride)
        cap = max(S * hs * ws, 1)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        ws_bytes = abi.scene_workspace_bytes(S, H, W)
        o = dict(hit=z((S, H, W), torch.int32), image=z((S, H, W, 3), torch.uint8), points=z((cap, 6), torch.float64),
                 point_pixel=z((cap,), torch.int32), scene_offsets=z((S + 1,), torch.int64),
                 visible=z((S, abi.SCENE_MAX_OBJECTS), torch.int32), vis_box=z((S, abi.SCENE_MAX_OBJECTS, 4), torch.int32))
        work = z((max(ws_bytes // 8, 1),), torch.int64)
        ptr = lambda x, T: C.cast(C.c_void_p(0 if x is None else x.data_ptr()), C.POINTER(T))
        hp = lambda a, T: a.ctypes.data_as(C.POINTER(T))
        a = abi.SceneRaycastArgs(S, H, W, self.stride, self.seed & 0xFFFFFFFF, 0, ptr(t['rtilt'], C.c_double), ptr(t['K'], C.c_double),
                                 ptr(t['scene_id'], C.c_int32), ptr(t['room'], C.c_double), ptr(t['part_offsets'], C.c_int32),
                                 ptr(parts_t, abi.ScenePart), hp(room, C.c_double), hp(part_offsets, C.c_int32), hp(n_objects, C.c_int32),
                                 self.noise_a, self.p_drop, self.max_range, self.min_cos2, C.c_void_p(work.data_ptr()), ws_bytes, cap,
                                 ptr(o['hit'], C.c_int32), ptr(o['image'], C.c_uint8), ptr(o['points'], C.c_double),
                                 ptr(o['point_pixel'], C.c_int32), ptr(o['scene_offsets'], C.c_int64), ptr(o['visible'], C.c_int32),
                                 ptr(o['vis_box'], C.c_int32))
        cuda = dev.type == 'cuda'
        if cuda and timed:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
        abi.check(self.rt.lib.t3d_scene_raycast(C.byref(a), self.rt.stream()), 't3d_scene_raycast')
        if cuda and timed:
            ev[1].record()
        if on_device:
            if cuda and timed:
                ev[1].synchronize()
                self.last_kernel_ms = ev[0].elapsed_time(ev[1])
            return o
        n = int(o['scene_offsets'][S].item())             # the copy back starts here (synchronises)
        h = {k: (v[:n] if k in ('points', 'point_pixel') else v).cpu().numpy() for k, v in o.items()}
        if cuda and timed:
            self.last_kernel_ms = ev[0].elapsed_time(ev[1])
        return h


# ---- layout (host) ----------------------------------------------------------------------------------------------------------------------
def rtilt_of(pitch, roll):
    ca, sa, cb, sb = np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])


def _rect(obj, grow=0.0):
    """The four ground-plane corners of an object's label box."""
    c, s = np.cos(obj['theta']), np.sin(obj['theta'])
    ax, ay = np.array([c, s]) * (obj['l'] + grow), np.array([-s, c]) * (obj['w'] + grow)
    p = obj['centroid'][:2]
    return np.array([p + ax + ay, p + ax - ay, p - ax - ay, p - ax + ay])


def rects_overlap(a, b):
    """Separating axes of two ground-plane rectangles (touching counts as apart)."""
    for r in (a, b):
        for i in range(2):
            n = r[i + 1] - r[i]
            n = np.array([-n[1], n[0]])
            pa, pb = a @ n, b @ n
            if pa.max() <= pb.min() or pb.max() <= pa.min():
                return False
    return True


def project_corners(corners_cam, Rtilt, K):
    """Upright camera corners (compute_box_3d) -> (uv [8,2], depth [8]) by the extractor's projection."""
    up_depth = np.stack([corners_cam[:, 0], corners_cam[:, 2], -corners_cam[:, 1]], 1)
    cam = SD.flip_axis_to_camera(up_depth @ Rtilt)           # rows of (Rtilt^T p)^T
    uvw = cam @ K.T
    return uvw[:, :2] / uvw[:, 2:3], uvw[:, 2]


def _label_object(obj):
    """The object as SUNObject3d holds it (for compute_box_3d)."""
    import types
    return types.SimpleNamespace(heading_angle=-obj['theta'], l=obj['l'], w=obj['w'], h=obj['h'], centroid=obj['centroid'])


def _fits(obj, others, room, Rtilt, K, W, H):
    r = _rect(obj)
    if r[:, 0].min() < room[0] or r[:, 0].max() > room[1] or r[:, 1].min() < room[2] or r[:, 1].max() > room[3]:
        return False
    uv, depth = project_corners(SD.compute_box_3d(_label_object(obj)), Rtilt, K)
    if depth.min() < 0.3:
        return False
    if uv[:, 0].max() < 0 or uv[:, 0].min() > W or uv[:, 1].max() < 0 or uv[:, 1].min() > H:
        return False
    return not any(rects_overlap(r, _rect(o)) for o in others)


def _sized(rng, classname):
    l, w, h = type_mean_size[classname] * rng.uniform(0.85, 1.15, size=3) / 2.0
    return dict(classname=classname, l=float(l), w=float(w), h=float(h))


def _at_wall(rng, obj, room):
    """Puts the object's back to one of three walls (the far one twice as likely), heading into the room, with jitter."""
    wall = rng.choice(4)
    gap = rng.uniform(0.02, 0.15)
    if wall <= 1:      # far wall: front towards the camera
        theta, x, y = -np.pi / 2, rng.uniform(room[0] + obj['w'], room[1] - obj['w']), room[3] - obj['l'] - gap
    elif wall == 2:    # left wall
        theta, x, y = 0.0, room[0] + obj['l'] + gap, rng.uniform(1.0, room[3] - obj['w'])
    else:
        theta, x, y = np.pi, room[1] - obj['l'] - gap, rng.uniform(1.0, room[3] - obj['w'])
    obj['theta'] = float(theta + rng.normal(0, 0.06))
    obj['centroid'] = np.array([x, y, room[4] + obj['h']])


def _in_room(rng, obj, room):
    obj['theta'] = float(rng.choice([0.0, np.pi / 2, np.pi, -np.pi / 2]) + rng.normal(0, 0.06))
    obj['centroid'] = np.array([rng.uniform(room[0] + 0.8, room[1] - 0.8), rng.uniform(1.5, room[3] - 1.0), room[4] + obj['h']])


def object_parts(obj, owner, inset, rng):
    """The boxes of one object: the class's fractions of the label box shrunk towards its centre by `inset` on every side."""
    inner = np.maximum(np.array([obj['l'], obj['w'], obj['h']]) - inset, 1e-3)
    c, s = np.cos(obj['theta']), np.sin(obj['theta'])
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    base = np.clip(np.array(COLOURS[obj['classname']], np.float64) + rng.uniform(-25, 25, size=3), 0, 255)
    shapes = SHAPES[obj['classname']]
    out = np.zeros(len(shapes), PART_DTYPE)
    for k, (pc, ph) in enumerate(shapes):
        lo, hi = (np.array(pc, np.float64) - np.array(ph)) * inner, (np.array(pc, np.float64) + np.array(ph)) * inner
        out[k]['centre'] = obj['centroid'] + R @ ((lo + hi) / 2.0)
        out[k]['half'] = (hi - lo) / 2.0
        out[k]['cos_r'], out[k]['sin_r'] = c, s
        out[k]['colour'] = np.clip(base * (1.0 - 0.06 * (k % 3)), 0, 255)
        out[k]['owner'] = owner
    return out


def layout(seed, sid, W, H, max_objects=12, surface_inset=0.02):
    """One scene: {'id', 'Rtilt', 'K', 'room', 'objects': [{classname, centroid, l, w, h (half sizes), theta}], 'parts', 'n_objects'}."""
    rng = _stream(seed, sid, 1)
    width, depth, height = rng.uniform(3.5, 5.5), rng.uniform(4.0, 6.5), rng.uniform(2.4, 3.0)
    cam_h, back, dx = rng.uniform(1.0, 1.5), rng.uniform(0.3, 0.8), rng.uniform(-0.4, 0.4)
    room = np.array([-width / 2 + dx, width / 2 + dx, -back, depth - back, -cam_h, height - cam_h])
    Rtilt = rtilt_of(rng.uniform(-0.28, -0.08), rng.uniform(-0.03, 0.03))
    f = 529.5 * W / 730.0
    K = np.array([[f, 0, W / 2.0 - 0.5], [0, f, H / 2.0 - 0.5], [0, 0, 1]])
    max_objects = min(int(max_objects), abi.SCENE_MAX_OBJECTS)
    want = int(rng.randint(3, max(max_objects, 3) + 1))
    objects = []

    def place(obj, how):
        for _ in range(30):
            how(rng, obj, room)
            if _fits(obj, objects, room, Rtilt, K, W, H):
                objects.append(obj)
                return True
        return False

    tries = 0
    while len(objects) < want and tries < 6 * want:
        tries += 1
        name = CLASSES[rng.randint(len(CLASSES))]
        if name == 'chair' and rng.uniform() < 0.6:
            continue                                         # chairs come with tables below
        obj = _sized(rng, name)
        if not place(obj, _in_room if name in ('table', 'desk') and rng.uniform() < 0.6 else _at_wall):
            continue
        if name in ('table', 'desk') and rng.uniform() < 0.8:
            # a row of chairs along the side the table's front looks at, facing it, a hand apart
            t = obj
            ct, st = np.cos(t['theta']), np.sin(t['theta'])
            chairs = [_sized(rng, 'chair') for _ in range(int(rng.randint(1, 4)))]
            step = max(c['w'] for c in chairs) * 2 + rng.uniform(0.04, 0.15)
            for k, ch in enumerate(chairs):
                if len(objects) >= want:
                    break
                along = (k - (len(chairs) - 1) / 2.0) * step
                ahead = t['l'] + ch['l'] + rng.uniform(0.03, 0.2)
                ch['theta'] = float(t['theta'] + np.pi + rng.normal(0, 0.08))
                ch['centroid'] = np.array([t['centroid'][0] + ct * ahead - st * along, t['centroid'][1] + st * ahead + ct * along,
                                           room[4] + ch['h']])
                if _fits(ch, objects, room, Rtilt, K, W, H):
                    objects.append(ch)
    parts = [object_parts(o, k, surface_inset, rng) for k, o in enumerate(objects)]
    parts = np.concatenate(parts) if parts else np.zeros(0, PART_DTYPE)
    return dict(id=int(sid), Rtilt=Rtilt, K=K, room=room, objects=objects, parts=parts[:abi.SCENE_MAX_PARTS], n_objects=len(objects))


# ---- labels and the simulated detector (host) ---------------------------------------------------------------------------------------------
def label_line(obj, Rtilt, K, W, H):
    """The label_dimension line of an object: the 2-D box is the extent of its projected corners clipped to the image."""
    uv, _ = project_corners(SD.compute_box_3d(_label_object(obj)), Rtilt, K)
    x0, y0 = max(float(uv[:, 0].min()), 0.0), max(float(uv[:, 1].min()), 0.0)
    x1, y1 = min(float(uv[:, 0].max()), W - 1.0), min(float(uv[:, 1].max()), H - 1.0)
    c, s = np.cos(obj['theta']), np.sin(obj['theta'])
    cen = obj['centroid']
    return LABEL_LINE % (obj['classname'], x0, y0, max(x1 - x0, 1.0), max(y1 - y0, 1.0), cen[0], cen[1], cen[2], obj['w'], obj['l'], obj['h'],
                         c, -s, s, c, c, s)


def detect_2d(seed, sid, labels, visible, vis_box, W, H, stride, o):
    """The simulated detector's reports for one scene: [(classname, box (xmin, ymin, xmax, ymax), confidence)], labels in order, then
    background boxes."""
    rng = _stream(seed, sid, 2)
    out = []
    clip = lambda b: np.array([min(max(b[0], 0.0), W - 2.0), min(max(b[1], 0.0), H - 2.0), min(max(b[2], 1.0), W - 1.0), min(max(b[3], 1.0), H - 1.0)])

    def tidy(b):
        b = clip(b)
        b[2], b[3] = max(b[2], b[0] + 1.0), max(b[3], b[1] + 1.0)
        return b
    if o['det_from_labels']:
        return [(lab['object'].classname, np.array(lab['object'].box2d), 1.0) for lab in labels]
    full = max(o['det_full_visible'] * (-(-W // stride)) * (-(-H // stride)), 1.0)
    for lab in labels:
        k = lab['owner']
        f = min(1.0, visible[k] / full)
        draws = rng.uniform(size=4)
        jitter, beta, second = rng.normal(size=4), rng.beta(o['det_conf_a'], o['det_conf_b']), rng.uniform(size=4)
        if draws[0] < min(1.0, o['det_miss'] * (1.0 + o['det_miss_occluded'] * (1.0 - f))):
            continue
        b = vis_box[k].astype(np.float64) + np.array([0, 0, 1, 1])
        size = np.array([b[2] - b[0], b[3] - b[1], b[2] - b[0], b[3] - b[1]])
        name = LOOK_ALIKE[lab['object'].classname] if draws[1] < o['det_confuse'] else lab['object'].classname
        conf = float(beta * (0.5 + 0.5 * f))
        box = tidy(b + o['det_jitter'] * size * jitter)
        out.append((name, box, conf))
        if draws[2] < o['det_dup']:
            shift = o['det_dup_shift'] * size[:2] * (2 * second[:2] - 1)
            scale = 0.8 + 0.3 * second[2]
            cx, cy = (box[0] + box[2]) / 2 + shift[0], (box[1] + box[3]) / 2 + shift[1]
            hw, hh = (box[2] - box[0]) / 2 * scale, (box[3] - box[1]) / 2 * scale
            out.append((name, tidy(np.array([cx - hw, cy - hh, cx + hw, cy + hh])), float(conf * (0.4 + 0.5 * second[3]))))
    for _ in range(int(rng.poisson(o['det_fp_per_image']))):
        w, h = rng.uniform(0.08, 0.4) * W, rng.uniform(0.1, 0.5) * H
        x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
        out.append((CLASSES[rng.randint(len(CLASSES))], tidy(np.array([x, y, x + w, y + h])), float(rng.beta(1.0, 5.0) * 0.6)))
    return out


def det_lines(dets):
    return ''.join('%s -1 -10 -10 %.2f %.2f %.2f %.2f %.6f\n' % (n, b[0], b[1], b[2], b[3], p) for n, b, p in dets)


def depth_text(depth):
    """depth/%06d.txt: `%.4f` text."""
    buf = io.BytesIO()
    np.savetxt(buf, depth, fmt='%.4f')
    return buf.getvalue()


def calib_text(Rtilt, K):
    return ' '.join(repr(float(v)) for v in Rtilt.reshape(-1, order='F')) + '\n' + ' '.join(repr(float(v)) for v in K.reshape(-1, order='F')) + '\n'


def jpeg_bytes(image_rgb):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image_rgb).save(buf, format='JPEG', quality=92)
    return buf.getvalue()


class _Calibration:
    def __init__(self, Rtilt, K):
        self.Rtilt, self.K = Rtilt, K


class _MemoryDataset:
    """The four getters of sunrgbd_data.sunrgbd_object, served from a SceneSet.  The image is the decoded JPEG the writer would write;
    depth_decimals=4 gives the depth as its `%.4f` text reads."""

    def __init__(self, scene_set, depth_decimals=None):
        self.s, self.depth_decimals = scene_set, depth_decimals

    def get_image(self, idx):
        from PIL import Image
        with Image.open(io.BytesIO(self.s.scene(idx)['jpeg']())) as im:
            return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])

    def get_depth(self, idx):
        d = self.s.scene(idx)['depth']
        if self.depth_decimals is None:
            return d
        if self.depth_decimals != 4:
            raise ValueError('the depth files carry four decimals')
        return np.array(depth_text(d).split(), dtype=np.float64).reshape(-1, 6)

    def get_calibration(self, idx):
        sc = self.s.scene(idx)
        # what calib_text writes and Calibration reads: the same doubles (repr round-trips)
        return _Calibration(sc['Rtilt'], sc['K'])

    def get_label_objects(self, idx):
        return [lab['object'] for lab in self.s.scene(idx)['labels']]


class SceneSet:
    """Generated scenes in host memory.  scenes: [{'id', 'Rtilt', 'K', 'room', 'objects', 'parts', 'image' [H,W,3] uint8 RGB,
    'depth' [n,6], 'point_owner' [n] (the object ordinal of every depth point, -1 for the room), 'visible' [n_objects], 'vis_box',
    'labels': [{'line', 'object' (SUNObject3d), 'owner'}], 'detections': [(classname, box, confidence)]}]."""

    def __init__(self, scenes, flags):
        self.scenes, self.flags = list(scenes), dict(flags)
        self._by_id = {s['id']: s for s in self.scenes}

    @property
    def ids(self):
        return [s['id'] for s in self.scenes]

    def scene(self, idx):
        return self._by_id[int(idx)]

    def extend(self, other):
        self.scenes.extend(other.scenes)
        self._by_id.update(other._by_id)

    def dataset(self, depth_decimals=None):
        return _MemoryDataset(self, depth_decimals)

    def class_counts(self):
        c = collections.Counter(lab['object'].classname for s in self.scenes for lab in s['labels'])
        return {name: int(c.get(name, 0)) for name in CLASSES}

    def write_scene(self, root, idx):
        sc, tr = self.scene(idx), os.path.join(root, 'training')
        name = '%06d' % sc['id']
        with open(os.path.join(tr, 'image', name + '.jpg'), 'wb') as fh:
            fh.write(sc['jpeg']())
        with open(os.path.join(tr, 'calib', name + '.txt'), 'w') as fh:
            fh.write(calib_text(sc['Rtilt'], sc['K']))
        with open(os.path.join(tr, 'depth', name + '.txt'), 'wb') as fh:
            fh.write(depth_text(sc['depth']))
        with open(os.path.join(tr, 'label_dimension', name + '.txt'), 'w') as fh:
            fh.write(''.join(lab['line'] + '\n' for lab in sc['labels']))
        with open(os.path.join(root, 'det', name + '.txt'), 'w') as fh:
            fh.write(det_lines(sc['detections']))

    def write(self, root, val_share=0.2, test_share=0.0, workers=SD.MAX_WORKERS):
        """<root>/training/{image,calib,depth,label_dimension}/%06d.*, <root>/det/%06d.txt, the five index files and synth.json."""
        make_dirs(root)
        with ThreadPoolExecutor(max_workers=max(1, min(int(workers), SD.MAX_WORKERS))) as pool:
            for f in [pool.submit(self.write_scene, root, i) for i in self.ids]:
                f.result()
        write_index_files(root, self.ids, val_share, test_share)
        write_summary(root, self.flags, self.class_counts(), len(self.scenes))


def make_dirs(root):
    for sub in ('image', 'calib', 'depth', 'label_dimension'):
        os.makedirs(os.path.join(root, 'training', sub), exist_ok=True)
    os.makedirs(os.path.join(root, 'det'), exist_ok=True)


def split_ids(ids, val_share, test_share):
    """train, val, test: the ids in order, the last shares of them val and test."""
    ids = list(ids)
    n = len(ids)
    n_test = int(round(n * test_share))
    n_val = min(int(round(n * val_share)), n - n_test)
    n_train = n - n_val - n_test
    return ids[:n_train], ids[n_train:n_train + n_val], ids[n_train + n_val:]


def index_lists(ids, val_share, test_share):
    """The ids of the five index files of sunrgbd_data.ROI_SEG_FILES."""
    train, val, test = split_ids(ids, val_share, test_share)
    lists = {'train_data_idx.txt': train, 'val_data_idx.txt': val, 'test_data_idx.txt': test, 'trainval_data_idx.txt': train + val,
             'train_mini_data_idx.txt': train[:max(1, len(train) // 10)]}
    assert set(lists) == {f[0] for f in SD.ROI_SEG_FILES}
    return lists


def write_index_files(root, ids, val_share, test_share):
    for name, lst in index_lists(ids, val_share, test_share).items():
        with open(os.path.join(root, 'training', name), 'w') as fh:
            fh.write(''.join('%d\n' % i for i in lst))


def write_summary(root, flags, class_counts, n_scenes):
    with open(os.path.join(root, 'synth.json'), 'w') as fh:
        json.dump({'seed': flags.get('seed'), 'scenes': n_scenes, 'flags': flags, 'class_counts': class_counts}, fh, indent=1, sort_keys=True)


def _options(kw):
    o = dict(DEFAULTS)
    unknown = set(kw) - set(o)
    if unknown:
        raise TypeError('unknown options: %s' % sorted(unknown))
    o.update(kw)
    return o


def generate_batches(rt, ids, seed, batch_scenes=16, **kw):
    """SceneSets of consecutive batches of `ids` (see generate)."""
    o = _options(kw)
    W, H, stride = int(o['width']), int(o['height']), int(o['stride'])
    if rt is None:
        from .engine import Runtime
        rt = Runtime()
    caster = SceneCaster(rt, H, W, stride, seed, o['noise_a'], o['p_drop'], o['max_range'], float(o['min_cos']) ** 2)
    ids = [int(i) for i in ids]
    flags = dict(o, seed=int(seed))
    for b0 in range(0, len(ids), max(int(batch_scenes), 1)):
        lay = [layout(seed, sid, W, H, o['max_objects'], o['surface_inset']) for sid in ids[b0:b0 + max(int(batch_scenes), 1)]]
        r = caster.run(lay)
        scenes = []
        for s, sc in enumerate(lay):
            lo, hi = int(r['scene_offsets'][s]), int(r['scene_offsets'][s + 1])
            pix = r['point_pixel'][lo:hi]
            hit = r['hit'][s].reshape(-1)[pix]
            owners = sc['parts']['owner']
            sc['point_owner'] = np.where(hit >= 0, owners[np.clip(hit, 0, max(len(owners) - 1, 0))] if len(owners) else -1, -1).astype(np.int32)
            sc['depth'], sc['image'] = r['points'][lo:hi], r['image'][s]
            sc['visible'], sc['vis_box'] = r['visible'][s][:sc['n_objects']], r['vis_box'][s][:sc['n_objects']]
            sc['labels'] = []
            for k, obj in enumerate(sc['objects']):
                if sc['visible'][k] < o['min_visible']:
                    continue
                line = label_line(obj, sc['Rtilt'], sc['K'], W, H)
                sc['labels'].append({'line': line, 'object': SD.SUNObject3d(line), 'owner': k})
            sc['detections'] = detect_2d(seed, sc['id'], sc['labels'], sc['visible'], sc['vis_box'], W, H, stride, o)
            sc['jpeg'] = _once(jpeg_bytes, sc['image'])
            scenes.append(sc)
        yield SceneSet(scenes, flags)


def _once(fn, arg):
    box = []

    def get():
        if not box:
            box.append(fn(arg))
        return box[0]
    return get


def generate(rt, ids, seed, batch_scenes=16, **kw):
    """Scenes `ids` of `seed` as a SceneSet.  Options: DEFAULTS (the image size, the stride of the depth points, the sensor's noise and
    limits, the detector's rates).  rt=None: the HIP runtime."""
    out = None
    for part in generate_batches(rt, ids, seed, batch_scenes, **kw):
        if out is None:
            out = part
        else:
            out.extend(part)
    return out if out is not None else SceneSet([], dict(_options(kw), seed=int(seed)))


def write_frustum_files(scene_set, out_dir, val_share=0.2, test_share=0.0, rt=None, seed=0, log=print):
    """The five files of sunrgbd_data (ROI_SEG_FILES) from scenes in memory: extract_roi_seg(dataset=...), no scene file is read."""
    os.makedirs(out_dir, exist_ok=True)
    lists = index_lists(scene_set.ids, val_share, test_share)
    written = []
    for idx_name, out_name, augmentX in SD.ROI_SEG_FILES:
        res = SD.extract_roi_seg(None, lists[idx_name], 'training', augmentX=augmentX, perturb_box2d=augmentX > 1, seed=seed, rt=rt,
                                 dataset=scene_set.dataset())
        path = os.path.join(out_dir, out_name)
        save_zipped_pickle(res, path)
        log('%s: %d frustums' % (path, len(res[0])))
        written.append(path)
    return written


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--out', required=True, help='data set root: <out>/training/{image,calib,depth,label_dimension}, <out>/det, <out>/synth.json')
    p.add_argument('--scenes', type=int, default=100)
    p.add_argument('--first_id', type=int, default=1, help='id of the first scene')
    p.add_argument('--seed', type=int, default=0)
    for k, v in DEFAULTS.items():
        if isinstance(v, bool):
            p.add_argument('--' + k, action='store_true')
        else:
            p.add_argument('--' + k, type=type(v), default=v)
    p.add_argument('--val_share', type=float, default=0.2)
    p.add_argument('--test_share', type=float, default=0.0)
    p.add_argument('--batch_scenes', type=int, default=16)
    p.add_argument('--frustum_dir', default=None, help='also write the five frustum files of sunrgbd_data here, from memory')
    p.add_argument('--no_files', action='store_true', help='with --frustum_dir: do not write the scene files')
    return p


def main(argv=None, rt=None, log=print):
    FLAGS = parser().parse_args(argv)
    if rt is None:
        from .engine import Runtime
        rt = Runtime()
    ids = list(range(FLAGS.first_id, FLAGS.first_id + FLAGS.scenes))
    opts = {k: getattr(FLAGS, k) for k in DEFAULTS}
    keep = FLAGS.frustum_dir is not None
    everything = None
    if not FLAGS.no_files:
        make_dirs(FLAGS.out)
    else:
        os.makedirs(FLAGS.out, exist_ok=True)
    counts, n, flags = collections.Counter(), 0, None
    with ThreadPoolExecutor(max_workers=SD.MAX_WORKERS) as pool:
        pending = []
        for part in generate_batches(rt, ids, FLAGS.seed, FLAGS.batch_scenes, **opts):      # the device casts the next batch ...
            for f in pending:
                f.result()
            pending = [] if FLAGS.no_files else [pool.submit(part.write_scene, FLAGS.out, i) for i in part.ids]      # ... while this one is formatted
            counts.update(part.class_counts())
            n, flags = n + len(part.scenes), part.flags
            if keep:
                if everything is None:
                    everything = part
                else:
                    everything.extend(part)
        for f in pending:
            f.result()
    if not FLAGS.no_files:
        write_index_files(FLAGS.out, ids, FLAGS.val_share, FLAGS.test_share)
    write_summary(FLAGS.out, flags or dict(opts, seed=FLAGS.seed), {k: int(counts.get(k, 0)) for k in CLASSES}, n)
    log('%d scenes, %d labelled objects -> %s' % (n, sum(counts.values()), FLAGS.out))
    if keep and everything is not None:
        write_frustum_files(everything, FLAGS.frustum_dir, FLAGS.val_share, FLAGS.test_share, rt=rt, seed=FLAGS.seed, log=log)
    return FLAGS.out


if __name__ == '__main__':
    main()
