"""TEST INFRASTRUCTURE ONLY -- NumPy executable specification of t3d_scene_raycast (include/t3d.h, csrc/scene_synth.hip), on host
pointers, so that transferable3d_amd/synth_scenes.py runs end to end through Runtime(device='cpu', lib=FakeSceneLib()).  Every
expression is the header's, elementwise fp64 in the stated order; the part loop is the only loop over data."""
import ctypes as C

import numpy as np

from fake_frustum import mix
from fake_t3d import AbiSizeError, FakeLib, _struct, arr
from transferable3d_amd import abi

M64 = (1 << 64) - 1
DBL_MAX = np.finfo(np.float64).max
SHADES = np.array(abi.SCENE_SHADES)
PART_DTYPE = np.dtype([('centre', '<f8', 3), ('half', '<f8', 3), ('cos_r', '<f8'), ('sin_r', '<f8'), ('colour', '<f8', 3),
                       ('owner', '<i4'), ('reserved', '<i4')])
assert PART_DTYPE.itemsize == C.sizeof(abi.ScenePart)


def uniforms(seed, scene_id, pixel, j):
    """U_j of the header for an array of pixels."""
    base = (((seed & 0xFFFFFFFF) << 32) ^ (((scene_id & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & M64)) & M64
    with np.errstate(over='ignore'):
        b = np.uint64(base) ^ ((np.asarray(pixel, np.uint64) + np.uint64(1)) * np.uint64(0xC2B2AE3D27D4EB4F))
        x = (b ^ np.uint64(0x94D049BB133111EB)) + np.uint64(((j + 1) * 0xBF58476D1CE4E5B9) & M64)
    return (mix(x).astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def rays(R, K, H, W):
    """d [H*W, 3] of every pixel, row-major."""
    v, u = np.divmod(np.arange(H * W), W)
    cx, cy = (u.astype(np.float64) - K[2]) / K[0], (v.astype(np.float64) - K[5]) / K[4]
    q0, q1, q2 = cx, 1.0, -cy
    return np.stack([(R[3 * i] * q0 + R[3 * i + 1] * q1) + R[3 * i + 2] * q2 for i in range(3)], 1), u, v


def hit_part(part, d):
    """(hit, t_in, face, nd) of one part for the rays d [n, 3]."""
    c, s = part['cos_r'], part['sin_r']
    nx, ny = -part['centre'][0], -part['centre'][1]
    o = (c * nx + s * ny, c * ny - s * nx, -part['centre'][2])
    e = (c * d[:, 0] + s * d[:, 1], c * d[:, 1] - s * d[:, 0], d[:, 2])
    n = len(d)
    tin, tout = np.full(n, -DBL_MAX), np.full(n, DBL_MAX)
    face, nd, miss = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, bool)
    for k in range(3):
        h, ok = part['half'][k], o[k]
        zero = e[k] == 0.0
        if ok < -h or ok > h:
            miss |= zero
        with np.errstate(divide='ignore', invalid='ignore'):
            ta, tb = (-h - ok) / e[k], (h - ok) / e[k]
        pos = e[k] > 0.0
        tn, tf = np.where(pos, ta, tb), np.where(pos, tb, ta)
        up = ~zero & (tn > tin)
        tin = np.where(up, tn, tin)
        face = np.where(up, 2 * k + np.where(pos, 0, 1), face).astype(np.int32)
        nd = np.where(up, e[k], nd)
        tout = np.where(~zero & (tf < tout), tf, tout)
    return ~miss & (tin > 0.0) & (tin <= tout), tin, face, nd


def hit_room(room, d):
    n = len(d)
    t, face, nd, any_ = np.full(n, DBL_MAX), np.zeros(n, np.int32), np.zeros(n), np.zeros(n, bool)
    for k in range(3):
        nz = d[:, k] != 0.0
        pos = d[:, k] > 0.0
        with np.errstate(divide='ignore', invalid='ignore'):
            tw = np.where(pos, room[2 * k + 1], room[2 * k]) / d[:, k]
        up = nz & (tw < t)
        t = np.where(up, tw, t)
        face = np.where(up, 2 * k + np.where(pos, 1, 0), face).astype(np.int32)
        nd = np.where(up, d[:, k], nd)
        any_ |= nz
    return any_, t, face, nd


def shade(colour, face):
    with np.errstate(invalid='ignore'):
        x = colour * SHADES[face] + 0.5
        x = np.where(x < 0.0, 0.0, x)
        x = np.where(x > 255.0, 255.0, x)
    return x.astype(np.int32).astype(np.uint8)


def cast_scene(R, K, room, parts, H, W, max_range, min_cos2):
    """hit [H*W], image [H*W, 3], t [H*W], d [H*W, 3] (t meaningful where hit >= -1)."""
    d, u, v = rays(R, K, H, W)
    n = H * W
    best, t_best, face_best, nd_best = np.full(n, -1, np.int32), np.full(n, DBL_MAX), np.zeros(n, np.int32), np.zeros(n)
    for k in range(len(parts)):
        ok, t, face, nd = hit_part(parts[k], d)
        up = ok & ((best < 0) | (t < t_best))
        best, t_best = np.where(up, k, best).astype(np.int32), np.where(up, t, t_best)
        face_best, nd_best = np.where(up, face, face_best), np.where(up, nd, nd_best)
    wall, t_room, face_room, nd_room = hit_room(room, d)
    part = (best >= 0) & (~wall | (t_best <= t_room))
    surface = part | wall
    hit = np.where(part, best, np.where(wall, abi.SCENE_HIT_ROOM, abi.SCENE_HIT_INVALID)).astype(np.int32)
    t = np.where(part, t_best, t_room)
    nd = np.where(part, nd_best, nd_room)
    face = np.where(part, face_best, face_room)
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(invalid='ignore'):
        valid = surface & (t <= max_range) & (nd * nd >= min_cos2 * dd)
    hit = np.where(valid, hit, abi.SCENE_HIT_INVALID).astype(np.int32)
    image = np.zeros((n, 3), np.uint8)
    is_room = hit == abi.SCENE_HIT_ROOM
    image[is_room] = shade(abi.SCENE_ROOM_COLOUR, face[is_room])[:, None]
    on = hit >= 0
    if on.any():
        col = np.stack([parts[k]['colour'] for k in range(len(parts))])[hit[on]]
        image[on] = shade(col, face[on][:, None])
    return hit, image, t, d, u, v


def normal(u1, u2):
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def emit_scene(hit, image, t, d, u, v, W, stride, seed, scene_id, noise_a, p_drop):
    """(rows [n, 6], pixel [n]) of the emitted pixels, and the pieces of the noise bound: (d, t, g) of every row."""
    pix = v * W + u
    emit = (hit >= abi.SCENE_HIT_ROOM) & (u % stride == 0) & (v % stride == 0) & ~(uniforms(seed, scene_id, pix, 0) < p_drop)
    idx = np.nonzero(emit)[0]
    tt, dd = t[idx], d[idx]
    g = np.zeros(len(idx))
    m = tt
    if noise_a != 0.0:
        g = normal(uniforms(seed, scene_id, pix[idx], 1), uniforms(seed, scene_id, pix[idx], 2))
        m = tt + ((noise_a * (tt * tt)) * g)
    rows = np.concatenate([dd * m[:, None], image[idx].astype(np.float64) / 255.0], 1)
    return rows, pix[idx].astype(np.int32), (dd, tt, g)


def stats(hit, pixel, owners, u, v, H, W):
    """visible [64], vis_box [64, 4] of one scene."""
    MO = abi.SCENE_MAX_OBJECTS
    vis, box = np.zeros(MO, np.int32), np.tile(np.array([W, H, -1, -1], np.int32), (MO, 1))
    own = np.where(hit >= 0, owners[np.clip(hit, 0, max(len(owners) - 1, 0))] if len(owners) else -1, -1)
    emitted = np.zeros(H * W, bool)
    emitted[pixel] = True
    for o in np.unique(own[(own >= 0) & (own < MO)]):
        m = own == o
        box[o] = (u[m].min(), v[m].min(), u[m].max(), v[m].max())
        vis[o] = int((m & emitted).sum())
    return vis, box


def refusal(p):
    """The return code of the argument checks, in the library's order (0: the call goes ahead)."""
    need = ('rtilt', 'K', 'scene_id', 'room', 'part_offsets', 'room_host', 'part_offsets_host', 'n_objects_host', 'hit', 'image', 'points',
            'scene_offsets', 'visible', 'vis_box')
    if any(not getattr(p, k) for k in need) or p.reserved != 0:
        return -1
    S = p.n_scenes
    if S < 1 or S > 65535 or p.H < 1 or p.W < 1 or p.H * p.W > (1 << 24) or p.stride < 1:
        return -2
    po, nobj = arr(p.part_offsets_host, S + 1), arr(p.n_objects_host, S)
    if po[0] != 0:
        return -2
    cnt = np.diff(po)
    if (cnt < 0).any() or (cnt > abi.SCENE_MAX_PARTS).any() or (nobj < 0).any() or (nobj > abi.SCENE_MAX_OBJECTS).any():
        return -2
    if po[-1] > 0 and not p.parts:
        return -1
    room = arr(p.room_host, S, 6)
    if not ((room[:, 0::2] < 0.0) & (room[:, 1::2] > 0.0)).all():
        return -1
    if not p.p_drop >= 0.0 or not p.noise_a >= 0.0 or not p.max_range > 0.0 or not 0.0 <= p.min_cos2 <= 1.0:
        return -1
    if not p.workspace or p.workspace % 8 or p.workspace_bytes < abi.scene_workspace_bytes(S, p.H, p.W):
        return -1
    if p.points_capacity < S * (-(-p.H // p.stride)) * (-(-p.W // p.stride)):
        return -1
    return 0


class FakeSceneLib(FakeLib):
    def t3d_scene_raycast(self, a, stream):
        if not a:
            return -1
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        rc = refusal(p)
        if rc:
            return rc
        S, H, W = p.n_scenes, p.H, p.W
        R, K, room, sid = arr(p.rtilt, S, 9), arr(p.K, S, 9), arr(p.room, S, 6), arr(p.scene_id, S)
        po = arr(p.part_offsets, S + 1)
        n_parts = int(po[-1])
        parts = np.zeros(0, PART_DTYPE)
        if n_parts:
            buf = (C.c_char * (n_parts * PART_DTYPE.itemsize)).from_address(C.addressof(p.parts.contents))
            parts = np.frombuffer(buf, PART_DTYPE)
        hit, image = arr(p.hit, S, H * W), arr(p.image, S, H * W, 3)
        points, so = arr(p.points, p.points_capacity, 6), arr(p.scene_offsets, S + 1)
        pp = arr(p.point_pixel, p.points_capacity)
        visible, vis_box = arr(p.visible, S, abi.SCENE_MAX_OBJECTS), arr(p.vis_box, S, abi.SCENE_MAX_OBJECTS, 4)
        row = 0
        for s in range(S):
            sp = parts[po[s]:po[s + 1]]
            h, img, t, d, u, v = cast_scene(R[s], K[s], room[s], sp, H, W, p.max_range, p.min_cos2)
            rows, pixel, _ = emit_scene(h, img, t, d, u, v, W, p.stride, p.seed, int(sid[s]), p.noise_a, p.p_drop)
            hit[s], image[s] = h, img
            so[s] = row
            points[row:row + len(rows)] = rows
            if pp is not None:
                pp[row:row + len(rows)] = pixel
            row += len(rows)
            visible[s], vis_box[s] = stats(h, pixel, sp['owner'], u, v, H, W)
        so[S] = row
        return 0
