"""TEST INFRASTRUCTURE ONLY -- the cases and checkers of t3d_scene_floor and t3d_detect_floor, shared by tests/test_floor_cpu.py (through
the NumPy specification tests/fake_floor.py) and tests/test_floor_gpu.py (through libt3d.so).

Every output is compared with the specification as bytes: the header states the order of every fp64 sum and the specification
replicates it, so there is no tolerance to derive.  Every output lies between guard bands (guard_bands.py; 64-bit operands are laid over
an int32 allocation of their size, scene_check._guarded).  Scene sizes: 0, 1, one less than, exactly and one more than the 256 lanes
and the 4096-point chunk, three chunks, and one scene of 64 * 4096 + 4097 points, the smallest whose first workgroups walk two chunks."""
import ctypes as C

import numpy as np
import torch

import fake_floor as FF
import scene_check as SCK
from transferable3d_amd import abi

SIZES = (0, 1, 255, 256, 257, 4095, 4096, 4097, 8193)
BATCHES = {1: (4097,), 3: (257, 0, 8193), 9: SIZES}
TWO_ROUNDS = abi.SCENE_FLOOR_BLOCKS * abi.SCENE_FLOOR_CHUNK + 4097
SMALL = dict(FF.OPTIONS, min_inliers=1)              # the defaults but for min_inliers: a scene of a few points has a floor too


def options(**kw):
    o = dict(FF.OPTIONS, **kw)
    if 'bin' in kw and 'inv_bin' not in kw:
        o['inv_bin'] = 1.0 / o['bin']
    return o


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def room(seed, n, ld=3, floor_z=-1.2, share=0.3, a=0.0, b=0.0, noise=0.002):
    """n points: `share` of them on the plane z = a x + b y + floor_z (with noise), the rest clutter above it."""
    r = np.random.RandomState(seed)
    p = r.uniform(-1.0, 1.0, size=(n, ld))
    x, y = r.uniform(-2.0, 2.0, n), r.uniform(1.0, 5.0, n)
    on = r.uniform(size=n) < share
    z = np.where(on, a * x + b * y + floor_z + noise * r.normal(size=n), r.uniform(floor_z + 0.15, 1.0, n))
    p[:, 0], p[:, 1], p[:, 2] = x, y, z
    return p


def batch(sizes, ld, seed=0):
    scenes = [room(seed + 17 * k + n, n, ld, floor_z=-1.0 - 0.1 * (k % 5)) for k, n in enumerate(sizes)]
    return np.concatenate(scenes) if scenes else np.zeros((0, ld)), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def flat(n, z, seed, ld=3, xr=(-2.0, 2.0), yr=(1.0, 5.0)):
    r = np.random.RandomState(seed)
    p = r.uniform(-1.0, 1.0, size=(n, ld))
    p[:, 0], p[:, 1], p[:, 2] = r.uniform(*xr, n), r.uniform(*yr, n), z
    return p


def case_table():
    """A floor of 1000 points at -1.21 under a table plane of 3000 at -0.51: the lowest peak wins."""
    return np.concatenate([flat(3000, -0.51, 1), flat(1000, -1.21, 2)]), FF.OPTIONS


def case_share(n_floor):
    """4096 points, n_floor of them in one bin, the rest above the range: min_share 0.25 asks for exactly 1024."""
    return np.concatenate([flat(n_floor, -1.21, 3), flat(4096 - n_floor, 0.5, 4)]), options(min_share=0.25)


EDGE = options(z_lo=-2.0, z_hi=-1.0, bin=2.0 ** -6, n_bins=64, min_inliers=1, min_share=0.0, band=2.0 ** -7)


def case_edges():
    """Heights exactly on the bin edges of bin = 2^-6: z_lo itself (bin 0), every edge k, z_hi itself (excluded), one ulp below z_hi."""
    ks = np.concatenate([np.zeros(40), np.arange(64), np.full(30, 64), np.full(7, 33)])
    p = flat(len(ks), 0.0, 5)
    p[:, 2] = -2.0 + ks * 2.0 ** -6
    p = np.concatenate([p, flat(1, np.nextafter(-1.0, -2.0), 6)])
    return p, EDGE


def case_plateau():
    """200 points in bin 10 and 200 in bin 11 of the edge histogram: c3[10] == c3[11]; the lower bin wins."""
    p = np.concatenate([flat(200, -2.0 + 10.5 * 2.0 ** -6, 7), flat(200, -2.0 + 11.5 * 2.0 ** -6, 8)])
    return p, dict(EDGE, band=2.0 ** -5)


def case_not_finite(ld=6):
    p = room(9, 3000, ld)
    p[5::7, 0], p[3::11, 1], p[2::13, 2], p[1::17, 2] = np.nan, np.inf, -np.inf, np.nan
    if ld > 3:
        p[::2, 3:] = np.nan                                 # the columns behind z mean nothing
    return p, FF.OPTIONS


TILT = (np.tan(np.radians(2.0)) * np.cos(0.7), np.tan(np.radians(2.0)) * np.sin(0.7), -1.3)


def case_tilt(deg=2.0, n=5000):
    """A noise-free plane tilted by `deg` degrees over 2 m x 2 m."""
    a, b = np.tan(np.radians(deg)) * np.cos(0.7), np.tan(np.radians(deg)) * np.sin(0.7)
    p = flat(n, 0.0, 10, xr=(-1.0, 1.0), yr=(2.0, 4.0))
    p[:, 2] = a * p[:, 0] + b * p[:, 1] + TILT[2]
    return p, FF.OPTIONS


def case_strip():
    """The floor seen as a strip: its points are collinear in X, Y."""
    p = flat(2000, -1.21, 11)
    p[:, 1] = 2.0 * p[:, 0] + 5.0
    return np.concatenate([p, room(12, 2000, share=0.0)]), FF.OPTIONS


# ---- the calls, every output between guard bands -------------------------------------------------------------------------------------------
def _ptr(t, T):
    return C.cast(C.c_void_p(0 if t is None else t.data_ptr()), C.POINTER(T))


def run_scene_floor(rt, points, offsets, o=FF.OPTIONS):
    """t3d_scene_floor -> (plane [S, 8], counts [S, 4], hist [S, n_bins]) as host arrays."""
    dev, S, nb = rt.device, len(offsets) - 1, o['n_bins']
    pts = torch.from_numpy(np.ascontiguousarray(points, np.float64)).to(dev)
    if pts.numel() == 0:
        pts = torch.zeros(1, points.shape[1], dtype=torch.float64, device=dev)
    off = torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(dev)
    spec = dict(plane=(np.float64, (S, 8)), counts=(np.int32, (S, 4)), hist=(np.int32, (S, nb)))
    out, checks = {}, []
    for k, (dt, shape) in spec.items():
        out[k], chk = SCK._guarded(int(np.prod(shape)) * np.dtype(dt).itemsize, dev, k)
        checks.append(chk)
    wsb = abi.scene_floor_workspace_bytes(S)
    work, chk = SCK._guarded(wsb, dev, 'workspace')
    checks.append(chk)
    before = pts.clone()
    a = abi.SceneFloorArgs(S, points.shape[1], nb, _ptr(pts, C.c_double), _ptr(off, C.c_int64), o['z_lo'], o['z_hi'], o['bin'], o['inv_bin'],
                           o['min_share'], o['min_inliers'], 0, o['band'], o['max_slope2'], o['min_spread'], o['min_det_ratio'],
                           C.c_void_p(work.data_ptr()), wsb, _ptr(out['plane'], C.c_double), _ptr(out['counts'], C.c_int32),
                           _ptr(out['hist'], C.c_int32))
    abi.check(rt.lib.t3d_scene_floor(C.byref(a), rt.stream()), 't3d_scene_floor')
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    for chk in checks:
        chk()
    assert torch.equal(pts.view(torch.int64), before.view(torch.int64)), 'the points were written'
    return tuple(out[k].cpu().numpy().view(spec[k][0]).reshape(spec[k][1]).copy() for k in ('plane', 'counts', 'hist'))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare_scene_floor(got, want, what):
    for name, g, w in zip(('plane', 'counts', 'hist'), got, want):
        assert same(g, w), '%s: %s differs from the specification at %s\n got %s\nwant %s' % (
            what, name, np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else (g.shape, w.shape), g[g != w][:4] if g.shape == w.shape else '',
            w[g != w][:4] if g.shape == w.shape else '')


def check_scene_floor(rt, points, offsets, o, what):
    got = run_scene_floor(rt, points, offsets, o)
    want = specification(points, offsets, o)
    compare_scene_floor(got, want, what)
    return got


def specification(points, offsets, o):
    key = (points.shape, hash(points.tobytes()), tuple(offsets), repr(sorted(o.items())))
    if key not in _SPEC:
        _SPEC[key] = FF.scene_floor_batch(points, offsets, o)
    return _SPEC[key]


_SPEC = {}


def one(points):
    return points, np.array([0, len(points)], np.int64)


# ---- t3d_scene_floor against the specification ---------------------------------------------------------------------------------------------
def check_batch(rt, S, ld):
    points, offsets = batch(BATCHES[S], ld, seed=S)
    plane, counts, _ = check_scene_floor(rt, points, offsets, SMALL, 'S = %d, ld = %d' % (S, ld))
    for s, n in enumerate(BATCHES[S]):
        assert counts[s, 0] == n
        if n >= 255:
            assert counts[s, 3] in (0, abi.FLOOR_LEVEL) and abs(plane[s, 5] - (-1.0 - 0.1 * (s % 5))) < 0.02, (s, n, plane[s], counts[s])
        if n == 0:
            assert counts[s].tolist() == [0, 0, -1, abi.FLOOR_NONE] and not plane[s].any()


def check_two_rounds(rt):
    points = room(21, TWO_ROUNDS, 3)
    plane, counts, _ = check_scene_floor(rt, *one(points), FF.OPTIONS, 'a scene of %d points' % TWO_ROUNDS)
    assert counts[0, 3] == 0 and counts[0, 1] > 0.25 * TWO_ROUNDS and abs(plane[0, 2] + 1.2) < 1e-3


def check_constructed(rt):
    p, o = case_table()
    plane, counts, hist = check_scene_floor(rt, *one(p), o, 'a floor under a table')
    assert counts[0, 1] == 1000 and abs(plane[0, 5] + 1.21) < 1e-12 and hist[0].sum() == 4000, (plane, counts)
    for n_floor, found in ((1023, False), (1024, True)):
        p, o = case_share(n_floor)
        plane, counts, hist = check_scene_floor(rt, *one(p), o, 'a share of %d / 4096' % n_floor)
        assert (counts[0, 3] == abi.FLOOR_NONE) == (not found) and counts[0, 0] == 4096 and hist[0].sum() == n_floor, counts
        assert counts[0, 1] == (n_floor if found else 0) and (counts[0, 2] >= 0) == found
    p, o = case_edges()
    plane, counts, hist = check_scene_floor(rt, *one(p), o, 'heights on the bin edges')
    want = np.ones(64, np.int32)
    want[0], want[33], want[63] = 41, 8, 2
    assert np.array_equal(hist[0], want) and counts[0, 0] == len(p) == hist[0].sum() + 30, hist
    for z, n_extra, filled, bin_ in ((-2.99, 0, 0, 0), (-0.21, 0, 139, 138), (-2.99, 1000, 0, 0)):
        # every floor point in the lowest bin and bin 1 empty: c3[-1] is 0, not hist[0], so bin 0 itself wins; in the highest bin and
        # bin 138 empty: c3[138] == c3[139] and the lower one wins, whatever c3[140] is taken to be
        p = np.concatenate([flat(4000, z, 13), flat(4000, 0.5, 14), flat(n_extra, -1.5, 15)])
        plane, counts, hist = check_scene_floor(rt, *one(p), FF.OPTIONS, 'a floor wholly in bin %d' % filled)
        assert hist[0, filled] == 4000 and hist[0, 1] == hist[0, 138] == 0 and counts[0].tolist() == [8000 + n_extra, 4000, bin_, 0], counts
        assert abs(plane[0, 5] - z) < 1e-12
    p, o = case_plateau()
    plane, counts, hist = check_scene_floor(rt, *one(p), o, 'a plateau of two equal c3')
    assert hist[0, 10] == hist[0, 11] == 200 and counts[0, 2] == 10 and counts[0, 1] == 400, counts
    for ld in (3, 6):
        p, o = case_not_finite(ld)
        plane, counts, hist = check_scene_floor(rt, *one(p), o, 'rows that are not finite')
        fin = np.isfinite(p[:, :3]).all(1)
        assert counts[0, 0] == fin.sum() < len(p) and np.isfinite(plane).all() and counts[0, 3] == 0, counts
    p, o = case_tilt(2.0)
    plane, counts, _ = check_scene_floor(rt, *one(p), o, 'a tilt of 2 degrees')
    assert counts[0, 3] == 0 and np.abs(plane[0, :3] - np.array(TILT)).max() < 1e-9, (plane, counts)
    p, o = case_strip()
    plane, counts, _ = check_scene_floor(rt, *one(p), o, 'a strip')
    assert counts[0, 3] == abi.FLOOR_LEVEL and plane[0, 0] == 0.0 and plane[0, 1] == 0.0 and abs(plane[0, 2] + 1.21) < 1e-12, (plane, counts)
    p, o = case_tilt(8.0)
    plane, counts, _ = check_scene_floor(rt, *one(p), o, 'a tilt of 8 degrees under a limit of 5')
    assert counts[0, 3] in (abi.FLOOR_LEVEL, abi.FLOOR_NONE) and plane[0, 0] == 0.0 and plane[0, 1] == 0.0, (plane, counts)


def check_batch_independence(rt):
    """A scene alone, first and last in a batch, and repeated: the same bytes."""
    a, b, c = room(31, 5000, 6), room(32, 8193, 6), room(33, 300, 6)
    off = lambda *s: np.concatenate([[0], np.cumsum([len(x) for x in s])]).astype(np.int64)
    alone = run_scene_floor(rt, b, off(b), SMALL)
    again = run_scene_floor(rt, b, off(b), SMALL)
    first = run_scene_floor(rt, np.concatenate([b, a, c]), off(b, a, c), SMALL)
    last = run_scene_floor(rt, np.concatenate([a, c, b]), off(a, c, b), SMALL)
    twice = run_scene_floor(rt, np.concatenate([b, b]), off(b, b), SMALL)
    assert alone[1][0, 3] == 0 and alone[1][0, 1] > 1000
    for k in range(3):
        assert same(alone[k], again[k]) and same(alone[k][0], first[k][0]) and same(alone[k][0], last[k][2]), k
        assert same(alone[k][0], twice[k][0]) and same(alone[k][0], twice[k][1]), k


def check_scene_floor_refusals(lib):
    null = C.c_void_p(0)
    a = abi.SceneFloorArgs()
    a.struct_size -= 8
    assert lib.t3d_scene_floor(C.byref(a), null) == abi.ERR_ABI
    assert lib.t3d_scene_floor(None, null) == -1
    buf, ibuf = np.zeros(1 << 14), np.zeros(1 << 14, np.int32)
    Dp, Ip, Lp = buf.ctypes.data_as(abi.D), ibuf.ctypes.data_as(abi.I), C.cast(buf.ctypes.data_as(abi.D), abi.L)

    def call(**kw):
        f = dict(n_scenes=2, ld=3, points=Dp, scene_offsets=Lp, reserved=0, workspace=C.c_void_p(buf.ctypes.data), workspace_bytes=buf.nbytes,
                 plane=Dp, counts=Ip, hist=Ip, **FF.OPTIONS)
        f.update(kw)
        return lib.t3d_scene_floor(C.byref(abi.SceneFloorArgs(**f)), null)
    for k in ('points', 'plane'):
        assert call(**{k: abi.D()}) == -1, k
    for k in ('counts', 'hist'):
        assert call(**{k: abi.I()}) == -1, k
    assert call(scene_offsets=abi.L()) == -1 and call(workspace=null) == -1 and call(reserved=1) == -1
    assert call(workspace=C.c_void_p(buf.ctypes.data + 4)) == -1 and call(workspace_bytes=abi.scene_floor_workspace_bytes(2) - 1) == -1
    assert call(n_scenes=-1) == -1 and call(n_bins=0) == -1 and call(n_bins=-3) == -1
    for bad in (0.0, -0.02, float('nan'), float('inf')):
        assert call(bin=bad) == -1 and call(inv_bin=bad) == -1, bad
    assert call(z_hi=-3.0) == -1 and call(z_hi=-3.5) == -1 and call(z_lo=float('nan')) == -1
    assert call(min_share=-0.1) == -1 and call(min_share=1.5) == -1 and call(min_share=float('nan')) == -1 and call(min_inliers=-1) == -1
    for k in ('band', 'max_slope2', 'min_spread', 'min_det_ratio'):
        assert call(**{k: -1.0}) == -1 and call(**{k: float('nan')}) == -1, k
    assert call(n_bins=abi.SCENE_FLOOR_MAX_BINS + 1) == -2 and call(ld=2) == -2 and call(n_scenes=65536) == -2
    assert call(n_scenes=0) == 0 and call(n_scenes=0, workspace_bytes=0) == 0, 'no scene: nothing to do, and nothing is launched'


# ---- t3d_detect_floor ------------------------------------------------------------------------------------------------------------------------
DETECT_SIZES = (0, 1, 63, 64, 65, 257)
PLANES = np.array([[0.02, -0.01, -1.25, 0.1, 3.0, -1.28, 1e-6, -1.29], [0.0, 0.0, -1.1, 0.0, 2.5, -1.1, 4e-6, -1.11], [0.0] * 8])
COUNTS = np.array([[9000, 3000, 85, 0], [7000, 900, 94, abi.FLOOR_LEVEL], [500, 0, -1, abi.FLOOR_NONE]], np.int32)
MAX_SNAP = 0.3


def detections(n, seed=0):
    """Labels, corners and scene indices with every kind of row, by i % 8: 0-2 near their floor, 3 without a scene, 4 in the scene
    without a floor, 5 a label entry that is not finite, 6 far from the floor, 7 sunk by more than its height."""
    r = np.random.RandomState(seed + n)
    label = np.zeros((n, 7), np.float32)
    label[:, :3] = r.uniform(0.3, 1.6, (n, 3))
    label[:, 3], label[:, 5], label[:, 6] = r.uniform(-2, 2, n), r.uniform(1, 5, n), r.uniform(-3.1, 3.1, n)
    kind = np.arange(n) % 8
    index = np.where(kind == 3, -1, np.where(kind == 4, 2, np.arange(n) % 2)).astype(np.int32)
    pl = PLANES[np.clip(index, 0, 2)]
    yf = -((pl[:, 0] * label[:, 3] + pl[:, 1] * label[:, 5]) + pl[:, 2])
    gap = np.where(kind == 6, r.choice([-0.9, 0.7], n), np.where(kind == 7, -label[:, 0] - 0.05, r.uniform(-0.25, 0.25, n)))
    label[:, 4] = (yf - gap).astype(np.float32)
    bad = np.nonzero(kind == 5)[0]
    label[bad, bad % 7] = np.array([np.nan, np.inf, -np.inf], np.float32)[bad % 3]
    corners = r.normal(0, 2.0, (n, 8, 3)).astype(np.float32)
    return label, corners, index


def run_detect_floor(rt, label, corners, index, mode, max_snap=MAX_SNAP, planes=PLANES, counts=COUNTS, outputs=True):
    dev, n = rt.device, len(label)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = dict(label=up(label.reshape(-1)), corners=up(corners.reshape(-1)), index=up(index), planes=up(planes.reshape(-1)), counts=up(counts.reshape(-1)))
    before = {k: v.clone() for k, v in t.items()}
    spec = dict(gap=(np.float64, (n,)), flags=(np.int32, (n,)), label_out=(np.float32, (n, 7)), corners_out=(np.float32, (n, 8, 3)))
    out, checks = {}, []
    for k, (dt, shape) in spec.items():
        out[k], chk = SCK._guarded(int(np.prod(shape)) * np.dtype(dt).itemsize, dev, k)
        checks.append(chk)
    ptr = _ptr
    a = abi.DetectFloorArgs(n, len(planes), mode, ptr(t['label'], C.c_float), ptr(t['corners'], C.c_float), ptr(t['index'], C.c_int32),
                            ptr(t['planes'], C.c_double), ptr(t['counts'], C.c_int32), max_snap, 0, ptr(out['gap'], C.c_double),
                            ptr(out['flags'], C.c_int32), ptr(out['label_out'] if outputs else None, C.c_float),
                            ptr(out['corners_out'] if outputs else None, C.c_float))
    abi.check(rt.lib.t3d_detect_floor(C.byref(a), rt.stream()), 't3d_detect_floor')
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    for chk in checks:
        chk()
    for k, v in t.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), 'the input %s was written' % k
    return tuple(out[k].cpu().numpy().view(spec[k][0]).reshape(spec[k][1]).copy() for k in spec)


def check_detect_floor(rt, n, mode):
    if n == 0:                                                 # (an empty tensor has no address: the call still names its arrays)
        dev = rt.device
        one_ = torch.zeros(64, dtype=torch.float32, device=dev)
        i_ = torch.zeros(64, dtype=torch.int32, device=dev)
        d_ = torch.zeros(64, dtype=torch.float64, device=dev)
        a = abi.DetectFloorArgs(0, 3, mode, _ptr(one_, C.c_float), _ptr(one_, C.c_float), _ptr(i_, C.c_int32), _ptr(d_, C.c_double), _ptr(i_, C.c_int32),
                                MAX_SNAP, 0, _ptr(d_, C.c_double), _ptr(i_, C.c_int32), _ptr(one_, C.c_float), _ptr(one_, C.c_float))
        assert rt.lib.t3d_detect_floor(C.byref(a), rt.stream()) == 0
        assert not one_.any() and not i_.any() and not d_.any()
        return
    label, corners, index = detections(n)
    got = run_detect_floor(rt, label, corners, index, mode)
    want = FF.detect_floor(label, corners, index, PLANES, COUNTS, mode, MAX_SNAP)
    gap, flags, lo, co = got
    for name, g, w in zip(('gap', 'flags', 'label_out', 'corners_out'), got, want):
        assert same(g, w), 'n = %d, mode %d: %s differs from the specification at %s' % (n, mode, name, np.argwhere(g.view(np.uint8) != w.view(np.uint8))[:4].tolist())
    snapped = (flags & abi.DETECT_FLOOR_SNAPPED) != 0
    assert same(lo[~snapped], label[~snapped]) and same(co[~snapped], corners[~snapped]), 'a row that is not snapped is a copy'
    assert same(co[:, :, 0], corners[:, :, 0]) and same(co[:, :, 2], corners[:, :, 2]), 'x and z of every corner stay'
    assert same(lo[:, [1, 2, 3, 5, 6]], label[:, [1, 2, 3, 5, 6]])
    assert not snapped.any() if mode == 0 else True
    unknown = (flags & (abi.DETECT_FLOOR_NO_FLOOR | abi.DETECT_FLOOR_NOT_FINITE)) != 0
    assert np.array_equal(np.isnan(gap), unknown)
    if n >= 64:
        kinds = [abi.DETECT_FLOOR_NO_FLOOR, abi.DETECT_FLOOR_NOT_FINITE, abi.DETECT_FLOOR_TOO_FAR] + \
            ([abi.DETECT_FLOOR_INVERTED] if mode == 2 else []) + ([abi.DETECT_FLOOR_SNAPPED] if mode else [])
        for bit in kinds:
            assert (flags & bit).any(), 'no row with flag %d' % bit
        assert ((flags & abi.DETECT_FLOOR_NO_FLOOR) != 0).sum() >= 2 * (n // 8), 'rows without a scene and rows of the scene without a floor'
    if mode:
        yf = gap[snapped] + label[snapped, 4].astype(np.float64)
        assert np.array_equal(lo[snapped, 4], yf.astype(np.float32)) and snapped.sum() > 0
        if mode == 1:
            assert same(lo[snapped, 0], label[snapped, 0])
        else:                                                  # the top face stays, to the rounding of the two fp32 entries
            top0, top1 = label[snapped, 4].astype(np.float64) - label[snapped, 0], lo[snapped, 4].astype(np.float64) - lo[snapped, 0]
            assert np.abs(top1 - top0).max() <= 2.0 ** -23 * 8.0, np.abs(top1 - top0).max()
    if mode == 0:                                              # measuring needs no output boxes
        again = run_detect_floor(rt, label, corners, index, 0, outputs=False)
        assert same(again[0], gap) and same(again[1], flags)


def check_detect_floor_refusals(lib):
    null = C.c_void_p(0)
    a = abi.DetectFloorArgs()
    a.struct_size -= 8
    assert lib.t3d_detect_floor(C.byref(a), null) == abi.ERR_ABI
    assert lib.t3d_detect_floor(None, null) == -1
    buf, ibuf, fbuf = np.zeros(1 << 12), np.zeros(1 << 12, np.int32), np.zeros(1 << 12, np.float32)
    Dp, Ip, Fp = buf.ctypes.data_as(abi.D), ibuf.ctypes.data_as(abi.I), fbuf.ctypes.data_as(abi.F)

    def call(**kw):
        f = dict(n=4, n_scenes=2, mode=1, label=Fp, corners=Fp, scene_index=Ip, plane=Dp, counts=Ip, max_snap=0.3, reserved=0, gap=Dp, flags=Ip,
                 label_out=Fp, corners_out=Fp)
        f.update(kw)
        return lib.t3d_detect_floor(C.byref(abi.DetectFloorArgs(**f)), null)
    for k in ('label', 'corners', 'label_out', 'corners_out'):
        assert call(**{k: abi.F()}) == -1, k
    for k in ('scene_index', 'counts', 'flags'):
        assert call(**{k: abi.I()}) == -1, k
    assert call(plane=abi.D()) == -1 and call(gap=abi.D()) == -1 and call(reserved=1) == -1
    assert call(n=-1) == -1 and call(n_scenes=-1) == -1 and call(mode=3) == -1 and call(mode=-1) == -1
    assert call(max_snap=-0.1) == -1 and call(max_snap=float('nan')) == -1
    assert call(n=0) == 0 and call(n=0, mode=0, label_out=abi.F(), corners_out=abi.F()) == 0
