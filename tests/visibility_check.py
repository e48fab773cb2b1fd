"""TEST INFRASTRUCTURE ONLY -- the cases and checkers of t3d_scene_range and t3d_detect_visibility, shared by tests/test_visibility_cpu.py
(through the NumPy specification tests/fake_visibility.py) and tests/test_visibility_gpu.py (through libt3d.so).

Every output is compared with the specification as bytes: the header states every fp64 operation in its order, the specification
transcribes it, and everything that is summed is an integer, so there is no tolerance to derive.  Every output lies between guard bands
(scene_check._guarded); inputs are compared with their copies afterwards.

The constructed cameras have Rtilt = I and power-of-two focal lengths, so that a point built from (u, v, depth) projects back onto
exactly (u, v): a point "on a cell border" is on it.  With Rtilt = I the ray through the pixel (pu, pv) is g = ((pu - cx) / f,
(pv - cy) / f, 1) in upright camera coordinates, which is what the hand counts below are worked out with."""
import ctypes as C

import numpy as np
import torch

import fake_visibility as FV
import scene_check as SCK
from transferable3d_amd import abi
from transferable3d_amd.eval_det import get_3d_box

EMPTY = FV.EMPTY
F32 = lambda v: np.array([v], np.float32).view(np.uint32)[0]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _ptr(t, T):
    return C.cast(C.c_void_p(0 if t is None else t.data_ptr()), C.POINTER(T))


def calib(f, cx, cy, W=0.0, H=0.0, Rtilt=None):
    R = np.eye(3) if Rtilt is None else np.asarray(Rtilt, np.float64)
    return np.concatenate([R.reshape(9), [f, 0, cx, 0, f, cy, 0, 0, 1], [W, H]]).astype(np.float64)


# ---- the range map ---------------------------------------------------------------------------------------------------------------------
SMALL_CAM = calib(16.0, 13.5, 9.5, 27, 19)          # a 27 x 19 image: 7 x 5 cells of 4 pixels, the last column and row partial
CELL = 4


def point_at(cal, u, v, depth):
    """The depth point (Rtilt = I) that projects onto (u, v) at camera depth `depth`."""
    f, cx, cy = cal[9], cal[11], cal[14]
    return [(u - cx) / f * depth, depth, -((v - cy) / f * depth)]


def case_constructed(ld=3):
    """-> (points, expected cells {(cx, cy): depth}, (n_finite, n_binned, n_filled)), every row placed by hand:
    on the corner of four cells; at u = W = 27 (inside the partial last column, whose cells end at 28); at u = 28, u = -0.5 and v = 20
    (outside); behind the camera and at depth 0; a NaN and an infinite row; two points in one cell (the nearer wins); the partial last
    cell; a depth that rounds to +infinity as an fp32; and two rows that tie exactly."""
    rows = [point_at(SMALL_CAM, 8.0, 4.0, 2.0),            # cell (2, 1): a border belongs to the cell it opens
            point_at(SMALL_CAM, 27.0, 0.0, 4.0),           # cell (6, 0)
            point_at(SMALL_CAM, 28.0, 5.0, 2.0), point_at(SMALL_CAM, -0.5, 5.0, 2.0), point_at(SMALL_CAM, 5.0, 20.0, 2.0),
            point_at(SMALL_CAM, 5.0, 5.0, -1.0), [0.25, 0.0, 0.25],
            [np.nan, 1.0, 0.0], [0.0, np.inf, 0.0],
            point_at(SMALL_CAM, 5.0, 5.0, 3.0), point_at(SMALL_CAM, 6.5, 6.0, 2.5),      # cell (1, 1): 2.5
            point_at(SMALL_CAM, 26.5, 18.5, 1.5),          # cell (6, 4)
            [0.0, 1e300, 0.0],                             # (float)depth is +infinity: not binned
            point_at(SMALL_CAM, 13.5, 9.5, 1.25), point_at(SMALL_CAM, 13.5, 9.5, 1.25)]      # cell (3, 2), twice
    p = np.zeros((len(rows), ld))
    p[:, :3] = rows
    if ld > 3:
        p[:, 3:] = np.nan                                  # the columns behind z mean nothing
    cells = {(2, 1): 2.0, (6, 0): 4.0, (1, 1): 2.5, (6, 4): 1.5, (3, 2): 1.25}
    return p, cells, (len(rows) - 2, 7, 5)                 # 15 rows, two of them not finite; seven binned (1 + 1 + 2 + 1 + 2) into five cells


def random_scene(seed, n, ld, cal, W, H):
    """n points over and around a W x H image, a tenth of them not finite, a tenth behind the camera."""
    r = np.random.RandomState(seed)
    u, v, depth = r.uniform(-0.2 * W, 1.2 * W, n), r.uniform(-0.2 * H, 1.2 * H, n), r.uniform(0.5, 8.0, n)
    depth[r.uniform(size=n) < 0.1] *= -1.0
    q = np.stack([(u - cal[11]) / cal[9] * depth, depth, -((v - cal[14]) / cal[13] * depth)], 1)
    R = cal[:9].reshape(3, 3)
    p = r.uniform(-1, 1, (n, ld))
    p[:, :3] = q @ R.T                                     # d = Rtilt q
    bad = np.nonzero(r.uniform(size=n) < 0.1)[0]
    p[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf])[bad % 3]
    return p


TILTED = calib(40.3, 33.3, 17.2, 67, 35, Rtilt=[[0.9998, 0.0, -0.02], [0.003, 0.9888, 0.149], [0.0198, -0.1493, 0.9886]])
CAMS = ((SMALL_CAM, 27, 19), (TILTED, 67, 35), (calib(16.0, 13.5, 9.5), 27, 19))
SIZES = (0, 1, 255, 257, 4097)
BATCHES = {1: [(n,) for n in SIZES], 3: [(257, 0, 4097), (1, 255, 257)]}


def range_batch(sizes, ld, seed):
    """Scenes of `sizes` points, scene s with camera CAMS[s % 3] through calibration row S - 1 - s -> the arguments of run_scene_range."""
    S = len(sizes)
    scenes = [random_scene(seed + 31 * s + n, n, ld, CAMS[s % 3][0], *CAMS[s % 3][1:]) for s, n in enumerate(sizes)]
    cal = np.stack([CAMS[s % 3][0] for s in range(S)][::-1])
    index = np.arange(S, dtype=np.int32)[::-1].copy()
    dims, goff = FV.grids([CAMS[s % 3][1:] for s in range(S)], CELL)
    return dict(points=np.concatenate(scenes) if scenes else np.zeros((0, ld)), offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                calib=cal, calib_index=index, dims=dims, goff=goff, n_cells=int(goff[-1]), cell=CELL)


def run_scene_range(rt, points, offsets, calib, calib_index, dims, goff, n_cells, cell):
    """t3d_scene_range -> (range [n_cells] uint32, counts [S, 4] int32) as host arrays."""
    dev, S = rt.device, len(offsets) - 1
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt) if np.size(a) else np.zeros(4, dt)).to(dev)
    t = dict(points=up(points, np.float64), offsets=up(offsets, np.int64), calib=up(calib, np.float64), index=up(calib_index, np.int32),
             dims=up(dims, np.int32), goff=up(goff, np.int64))
    before = {k: v.clone() for k, v in t.items()}
    spec = dict(range=(np.uint32, (n_cells,)), counts=(np.int32, (S, 4)))
    out, checks = {}, []
    for k, (dt, shape) in spec.items():
        out[k], chk = SCK._guarded(int(np.prod(shape)) * np.dtype(dt).itemsize, dev, k)
        checks.append(chk)
    a = abi.SceneRangeArgs(S, points.shape[1], cell, len(np.asarray(calib).reshape(-1, 20)), _ptr(t['points'], C.c_double), _ptr(t['offsets'], C.c_int64),
                           _ptr(t['calib'], C.c_double), _ptr(t['index'], C.c_int32), _ptr(t['dims'], C.c_int32), _ptr(t['goff'], C.c_int64), n_cells, 0,
                           _ptr(out['range'], C.c_uint32), _ptr(out['counts'], C.c_int32))
    abi.check(rt.lib.t3d_scene_range(C.byref(a), rt.stream()), 't3d_scene_range')
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    for chk in checks:
        chk()
    for k, v in t.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), 'the input %s was written' % k
    return tuple(out[k].cpu().numpy().view(spec[k][0]).reshape(spec[k][1]).copy() for k in spec)


def check_scene_range(rt, b, what):
    got = run_scene_range(rt, **b)
    want = FV.scene_range_batch(b['points'], b['offsets'], b['calib'], b['calib_index'], b['dims'], b['goff'], b['n_cells'], b['cell'])
    for name, g, w in zip(('range', 'counts'), got, want):
        assert same(g, w), '%s: %s differs from the specification at %s' % (what, name, np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else (g.shape, w.shape))
    return got


def check_range_batch(rt, S, ld):
    for k, sizes in enumerate(BATCHES[S]):
        b = range_batch(sizes, ld, seed=100 * S + k)
        rng, counts = check_scene_range(rt, b, 'S = %d, ld = %d, sizes %s' % (S, ld, sizes))
        for s, n in enumerate(sizes):
            cells = rng[b['goff'][s]:b['goff'][s + 1]]
            assert counts[s, 3] == 0 and counts[s, 0] <= n and counts[s, 2] == (cells != EMPTY).sum() <= counts[s, 1] <= counts[s, 0], counts[s]
            if n >= 255:
                assert 0 < counts[s, 2] and counts[s, 1] < counts[s, 0] < n, counts[s]
            if n == 0:
                assert not counts[s].any() and (cells == EMPTY).all()


def check_range_constructed(rt):
    for ld in (3, 6):
        p, cells, want_counts = case_constructed(ld)
        dims, goff = FV.grids([(27, 19)], CELL)
        assert dims.tolist() == [[7, 5]]
        rng, counts = check_scene_range(rt, dict(points=p, offsets=np.array([0, len(p)], np.int64), calib=SMALL_CAM[None], calib_index=np.zeros(1, np.int32),
                                                 dims=dims, goff=goff, n_cells=35, cell=CELL), 'the constructed scene, ld = %d' % ld)
        want = np.full(35, EMPTY, np.uint32)
        for (cx, cy), depth in cells.items():
            want[cy * 7 + cx] = F32(depth)
        assert same(rng, want), (rng.view(np.float32).reshape(5, 7), want.view(np.float32).reshape(5, 7))
        assert counts[0].tolist() == list(want_counts) + [0], counts


def check_range_flags(rt):
    """A scene without a calibration row and scenes whose grids do not fit: counted, flagged, and no cell is written for them."""
    b = range_batch((257, 255, 257, 255), 3, seed=7)
    b['calib_index'][1] = -1
    b['dims'][2] = (0, 5)
    b['goff'][3] = b['n_cells'] - 1
    rng, counts = check_scene_range(rt, b, 'flagged scenes')
    assert counts[:, 3].tolist() == [0, abi.RANGE_NO_CALIB, abi.RANGE_BAD_GRID, abi.RANGE_BAD_GRID] and (counts[1:, 1:3] == 0).all() and (counts[:, 0] > 200).all()
    assert (rng[b['goff'][1]:] == EMPTY).all() and (rng[:b['goff'][1]] != EMPTY).any()


def check_range_batch_independence(rt):
    """A scene alone, first and last in a batch, and repeated: the same cells and the same counts."""
    cams = [CAMS[1], CAMS[0], CAMS[1]]
    scenes = [random_scene(41 + k, n, 6, cams[k][0], *cams[k][1:]) for k, n in enumerate((4097, 300, 900))]

    def run(order):
        dims, goff = FV.grids([cams[k][1:] for k in order], CELL)
        pts = np.concatenate([scenes[k] for k in order])
        off = np.concatenate([[0], np.cumsum([len(scenes[k]) for k in order])]).astype(np.int64)
        rng, counts = run_scene_range(rt, pts, off, np.stack([cams[k][0] for k in order]), np.arange(len(order), dtype=np.int32), dims, goff, int(goff[-1]), CELL)
        return [(rng[goff[j]:goff[j + 1]], counts[j]) for j in range(len(order))]
    alone, again = run([0])[0], run([0])[0]
    first, last, twice = run([0, 1, 2])[0], run([1, 2, 0])[2], run([0, 0])
    assert alone[1][1] > 1000 and alone[1][2] > 50
    for other in (again, first, last, twice[0], twice[1]):
        assert same(alone[0], other[0]) and same(alone[1], other[1])


def check_scene_range_refusals(lib):
    null = C.c_void_p(0)
    a = abi.SceneRangeArgs()
    a.struct_size -= 8
    assert lib.t3d_scene_range(C.byref(a), null) == abi.ERR_ABI
    assert lib.t3d_scene_range(None, null) == -1
    buf, ibuf = np.zeros(1 << 12), np.zeros(1 << 12, np.int32)
    Dp, Ip, Lp, Up = buf.ctypes.data_as(abi.D), ibuf.ctypes.data_as(abi.I), C.cast(buf.ctypes.data_as(abi.D), abi.L), C.cast(ibuf.ctypes.data_as(abi.I), abi.U32)

    def call(**kw):
        f = dict(n_scenes=2, ld=3, cell=4, n_calib=2, points=Dp, scene_offsets=Lp, calib=Dp, calib_index=Ip, grid_dims=Ip, grid_offsets=Lp, n_cells=64,
                 reserved=0, range=Up, counts=Ip)
        f.update(kw)
        return lib.t3d_scene_range(C.byref(abi.SceneRangeArgs(**f)), null)
    for k in ('points', 'calib'):
        assert call(**{k: abi.D()}) == -1, k
    for k in ('calib_index', 'grid_dims', 'counts'):
        assert call(**{k: abi.I()}) == -1, k
    for k in ('scene_offsets', 'grid_offsets'):
        assert call(**{k: abi.L()}) == -1, k
    assert call(range=abi.U32()) == -1 and call(reserved=1) == -1 and call(n_scenes=-1) == -1 and call(cell=0) == -1 and call(cell=-4) == -1
    assert call(n_calib=-1) == -1 and call(n_cells=-1) == -1
    assert call(ld=2) == -2 and call(n_scenes=65536) == -2 and call(n_cells=2 ** 31) == -2
    assert call(n_scenes=0) == 0 and call(n_scenes=0, n_cells=0, range=abi.U32()) == 0, 'no scene: nothing to do, and nothing is launched'
    assert not buf.any() and not ibuf.any()


# ---- the boxes -------------------------------------------------------------------------------------------------------------------------
WALL_CAM = calib(32.0, 48.0, 40.0, 96, 80)          # 96 x 80: 24 x 20 cells; cell centres at 2, 6, 10, ...: 46 and 50 around the axis
GW, GH = 24, 20
OFFSETS = {1: np.zeros(1), 3: np.array([-0.125, 0.0, 0.125]), 9: (np.arange(9) - 4) * 0.03125}
MARGIN, MIN_CHORD, MIN_GAIN = 0.05, 0.1, 4


def box(centre, lx, hy, wz, ry=0.0):
    """(label (h, w, l, tx, ty, tz, ry), corners [8, 3]) fp32 of the box at `centre` (upright camera: x right, y down, z forward) with
    extents lx, hy, wz along x, y, z at ry = 0 -- as the decode writes them: ty is the bottom."""
    corners = get_3d_box((lx, wz, hy), ry, centre).astype(np.float32)
    return np.array([hy, wz, lx, centre[0], centre[1] + hy / 2.0, centre[2], ry], np.float32), corners


def wall(depth=5.0):
    return np.full(GW * GH, F32(depth), np.uint32)


def hand_cases():
    """[(what, label, corners, map, expected profile row of the box itself (rays, unknown, front, inside, through, graze))].

    The box is 2.2 wide, 2 high and 1 deep, centred on the axis at depth z0, so it spans t in [z0 - 0.5, z0 + 0.5].  The ray through the
    column pu leaves its sides at t = 1.1 * 32 / |pu - 48|: 17.6 for the columns 46 and 50, 5.87 for 42 and 54, 3.52 for 38 and 58,
    2.51 for 34 and 62;  through the row pv it leaves top and bottom at t = 32 / |pv - 40|: 16 for the rows 38 and 42, 5.33 for 34
    and 46, 3.2 for 30 and 50.
      z0 = 4   (t in [3.5, 4.5]): columns 42 .. 54 and rows 34 .. 46 cross it whole: 16 rays; columns 38 and 58 clip 0.02 of it in
               these four rows: 8 grazes.  The wall at 5 lies behind 4.5 + 0.05: all through.
      z0 = 5   (t in [4.5, 5.5]): the same 16 (rows 34 and 46 cross 0.83 of it), no graze; the wall lies inside.
      z0 = 6.5 (t in [6, 7]): columns 46, 50 and rows 38, 42 only: 4 rays; the wall lies in front of 6 - 0.05.
      a hole: the cells of (46, 38) and (50, 42) -- (11, 9) and (12, 10) -- empty under the box at 4: 2 unknown, 14 through."""
    cases = []
    for what, z0, m, want in (('in front of the wall', 4.0, wall(), (16, 0, 0, 0, 16, 8)), ('around the wall', 5.0, wall(), (16, 0, 0, 16, 0, 0)),
                              ('behind the wall', 6.5, wall(), (4, 0, 4, 0, 0, 0))):
        cases.append((what,) + box((0.0, 0.0, z0), 2.2, 2.0, 1.0) + (m, want))
    m = wall()
    m[9 * GW + 11] = m[10 * GW + 12] = EMPTY
    cases.append(('a hole in the map',) + box((0.0, 0.0, 4.0), 2.2, 2.0, 1.0) + (m, (16, 2, 0, 0, 14, 8)))
    return cases


def rect_cells(label, corners, cal=WALL_CAM, gw=GW, gh=GH):
    """How many cells the rectangle of a box covers (the specification's own fold and clip)."""
    X, Y, Z = (corners[:, k].astype(np.float64) for k in range(3))
    u, v, _ = FV.project(cal, X, Z, -Y)
    cx0, cx1 = max(int(np.floor(u.min() / CELL)), 0), min(int(np.floor(u.max() / CELL)), gw - 1)
    cy0, cy1 = max(int(np.floor(v.min() / CELL)), 0), min(int(np.floor(v.max() / CELL)), gh - 1)
    return (cx1 - cx0 + 1) * (cy1 - cy0 + 1)


def special_rows():
    """[(what, label, corners, scene index)]: rows 0-9 of every detection batch of two or more... (`detections` places them)."""
    rows = []
    rows.append(('exactly 256 cells',) + box((0.0, 0.0, 4.0), 2 * 30 * 3.5 / 32, 2 * 30 * 3.5 / 32, 1.0) + (0,))
    rows.append(('324 cells: the loop over the cells runs twice',) + box((0.0, 0.0, 4.0), 2 * 34 * 3.5 / 32, 2 * 34 * 3.5 / 32, 1.0) + (0,))
    rows.append(('outside the image',) + box((12.0, 0.0, 4.0), 1.0, 1.0, 1.0) + (0,))
    rows.append(('a corner behind the camera',) + box((0.0, 0.0, 0.3), 1.0, 1.0, 1.0) + (0,))
    rows.append(('a zero-length edge',) + box((0.2, 0.1, 4.0), 1.0, 0.0, 1.0) + (0,))
    lab, kor = box((0.0, 0.0, 4.0), 1.0, 1.0, 1.0)
    lab[1] = np.nan
    rows.append(('a NaN label', lab, kor, 0))
    lab, kor = box((0.0, 0.0, 4.0), 1.0, 1.0, 1.0)
    kor[5, 2] = np.inf
    rows.append(('an infinite corner', lab, kor, 0))
    rows.append(('no scene',) + box((0.0, 0.0, 4.0), 1.0, 1.0, 1.0) + (-1,))
    rows.append(('a scene whose grid does not fit',) + box((0.0, 0.0, 4.0), 1.0, 1.0, 1.0) + (2,))
    rows.append(('a tie of the candidates either side',) + box((0.0, 0.0, 4.0), 1.0, 1.0, 1.0) + (0,))
    rows.append(('turned, off the axis',) + box((-0.7, 0.3, 4.6), 1.4, 0.9, 0.8, 0.6) + (1,))
    return rows


def tie_wall():
    """The wall at 5 but for the four cells on the axis: 3.2, 3.2, 4.8 and none.  The box of side 1 at depth 4 and its candidates at 3.5 and
    4.5 (K = 3) are crossed by the rays of exactly these four cells (the columns 42 and 54 leave the nearest candidate's sides at
    t = 0.5 * 32 / 6 = 2.67, in front of it).  A return at 3.2 lies inside [3, 4] and in front of the other two; one at 4.8 lies behind
    [3, 4] and [3.5, 4.5] and inside [4, 5]: the scores are +1, -1, +1."""
    m = wall()
    m[9 * GW + 11] = m[9 * GW + 12] = F32(3.2)
    m[10 * GW + 11] = F32(4.8)
    m[10 * GW + 12] = EMPTY
    return m


def coarse_map(seed):
    """Depths of a few levels over blocks of 3 x 3 cells, a fifth of the blocks empty: scores that tie."""
    r = np.random.RandomState(seed)
    levels = np.array([EMPTY, F32(3.0), F32(4.5), F32(4.5), F32(6.0)], np.uint32)
    blocks = levels[r.randint(0, 5, ((GH + 2) // 3, (GW + 2) // 3))]
    return np.repeat(np.repeat(blocks, 3, 0), 3, 1)[:GH, :GW].reshape(-1).copy()


def world(seed=0):
    """Three scenes: 0 the wall at 5; 1 a coarse map of levels under the tilted camera's frame (same image size); 2 a grid that does
    not fit.  -> (calib [3, 20], dims, goff, range)."""
    cal = np.stack([WALL_CAM, calib(32.0, 47.0, 41.0, 96, 80, Rtilt=TILTED[:9].reshape(3, 3)), WALL_CAM])
    dims = np.array([[GW, GH], [GW, GH], [GW, GH]], np.int32)
    goff = np.array([0, GW * GH, 2 * GW * GH - 5, 3 * GW * GH], np.int64)
    return cal, dims, goff, np.concatenate([tie_wall(), coarse_map(seed)])


def detections(n, seed=0):
    """n rows: the special rows first (as many as fit), then random boxes in front of, around and behind what scenes 0 and 1 show."""
    r = np.random.RandomState(seed + n)
    label, corners, index = np.zeros((n, 7), np.float32), np.zeros((n, 8, 3), np.float32), np.zeros(n, np.int32)
    special = special_rows()
    for i in range(n):
        if i < len(special) and n >= 2:
            _, label[i], corners[i], index[i] = special[i]
        else:
            z0 = r.choice([3.0, 4.0, 4.5, 5.0, 6.0]) + r.uniform(-0.3, 0.3)
            label[i], corners[i] = box((r.uniform(-1.5, 1.5), r.uniform(-1.0, 1.0), z0), r.uniform(0.3, 2.0), r.uniform(0.3, 1.5), r.uniform(0.3, 1.5), r.uniform(-3.1, 3.1))
            index[i] = i % 2
    return label, corners, index


def run_detect_visibility(rt, label, corners, index, cal, dims, goff, range_, offsets, mode, margin=MARGIN, min_chord=MIN_CHORD, min_gain=MIN_GAIN,
                          outputs=True, cell=CELL):
    dev, n, K = rt.device, len(label), len(offsets)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a).reshape(-1)).to(dev)
    t = dict(label=up(label), corners=up(corners), index=up(index), calib=up(cal), dims=up(dims), goff=up(goff), range=up(range_))
    before = {k: v.clone() for k, v in t.items()}
    spec = dict(profile=(np.int32, (n, K, 6)), measures=(np.float64, (n, 3)), choice=(np.int32, (n,)), flags=(np.int32, (n,)),
                label_out=(np.float32, (n, 7)), corners_out=(np.float32, (n, 8, 3)))
    out, checks = {}, []
    for k, (dt, shape) in spec.items():
        out[k], chk = SCK._guarded(int(np.prod(shape)) * np.dtype(dt).itemsize, dev, k)
        checks.append(chk)
    o = (C.c_double * abi.VIS_MAX_OFFSETS)(*[float(v) for v in offsets])
    a = abi.DetectVisibilityArgs(n, len(dims), mode, K, cell, min_gain, 0, _ptr(t['label'], C.c_float), _ptr(t['corners'], C.c_float), _ptr(t['index'], C.c_int32),
                                 _ptr(t['calib'], C.c_double), _ptr(t['dims'], C.c_int32), _ptr(t['goff'], C.c_int64), _ptr(t['range'], C.c_uint32), len(range_),
                                 margin, min_chord, o, _ptr(out['profile'], C.c_int32), _ptr(out['measures'], C.c_double), _ptr(out['choice'], C.c_int32),
                                 _ptr(out['flags'], C.c_int32), _ptr(out['label_out'] if outputs else None, C.c_float),
                                 _ptr(out['corners_out'] if outputs else None, C.c_float))
    abi.check(rt.lib.t3d_detect_visibility(C.byref(a), rt.stream()), 't3d_detect_visibility')
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    for chk in checks:
        chk()
    for k, v in t.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), 'the input %s was written' % k
    return tuple(out[k].cpu().numpy().view(spec[k][0]).reshape(spec[k][1]).copy() for k in spec)


NAMES = ('profile', 'measures', 'choice', 'flags', 'label_out', 'corners_out')


def compare(got, want, what, names=NAMES):
    for name, g, w in zip(names, got, want):
        assert same(g, w), '%s: %s differs from the specification at %s' % (what, name, np.argwhere(g.view(np.uint8) != w.view(np.uint8))[:4].tolist() if g.shape == w.shape else (g.shape, w.shape))


def check_hand_cases(rt):
    """The one-wall scenes with the counts written by hand, measured alone (K = 1) and as the middle of nine candidates."""
    for what, label, corners, m, want in hand_cases():
        for K in (1, 9):
            got = run_detect_visibility(rt, label[None], corners[None], np.zeros(1, np.int32), WALL_CAM[None], np.array([[GW, GH]], np.int32),
                                        np.array([0, GW * GH], np.int64), m, OFFSETS[K], 0)
            compare(got, FV.detect_visibility(label[None], corners[None], [0], WALL_CAM[None], [[GW, GH]], [0, GW * GH], m, CELL, OFFSETS[K], MARGIN, MIN_CHORD, MIN_GAIN, 0),
                    '%s, K = %d' % (what, K))
            profile, measures, choice, flags = got[:4]
            mid = (K - 1) // 2
            assert tuple(profile[0, mid]) == want, (what, K, profile[0, mid], want)
            rays, unknown, front, inside, through, graze = want
            seen = through + inside
            assert measures[0].tolist() == [through / seen if seen else 0.0, front / rays, inside / rays], (what, measures)
            assert flags[0] == (0 if seen else abi.VIS_NO_EVIDENCE), (what, flags)


def check_detect_visibility(rt, n, K, mode):
    if n == 0:                                                 # (an empty tensor has no address: the call still names its arrays)
        dev = rt.device
        f_, i_, d_ = (torch.zeros(64, dtype=dt, device=dev) for dt in (torch.float32, torch.int32, torch.float64))
        o = (C.c_double * abi.VIS_MAX_OFFSETS)(*[float(v) for v in OFFSETS[K]])
        a = abi.DetectVisibilityArgs(0, 1, mode, K, CELL, MIN_GAIN, 0, _ptr(f_, C.c_float), _ptr(f_, C.c_float), _ptr(i_, C.c_int32), _ptr(d_, C.c_double),
                                     _ptr(i_, C.c_int32), _ptr(d_, C.c_int64), _ptr(i_, C.c_uint32), 16, MARGIN, MIN_CHORD, o, _ptr(i_, C.c_int32),
                                     _ptr(d_, C.c_double), _ptr(i_, C.c_int32), _ptr(i_, C.c_int32), _ptr(f_, C.c_float), _ptr(f_, C.c_float))
        assert rt.lib.t3d_detect_visibility(C.byref(a), rt.stream()) == 0
        assert not f_.any() and not i_.any() and not d_.any()
        return
    label, corners, index = detections(n)
    cal, dims, goff, range_ = world()
    got = run_detect_visibility(rt, label, corners, index, cal, dims, goff, range_, OFFSETS[K], mode)
    want = specification(n, K, mode)
    compare(got, want, 'n = %d, K = %d, mode %d' % (n, K, mode))
    profile, measures, choice, flags, lo, co = got
    mid = (K - 1) // 2
    moved = (flags & abi.VIS_SNAPPED) != 0
    assert same(lo[~moved], label[~moved]) and same(co[~moved], corners[~moved]), 'a row that did not move is a copy'
    assert same(lo[:, [0, 1, 2, 4, 6]], label[:, [0, 1, 2, 4, 6]]) and same(co[:, :, 1], corners[:, :, 1]), 'a slide moves x and z alone'
    assert not (moved.any() and (mode == 0 or K == 1)), 'nothing moves where nothing is asked to or no candidate exists'
    assert (profile[:, :, 0] == profile[:, :, 1:5].sum(2)).all()
    if n >= 2:
        what = [r[0] for r in special_rows()][:n]
        row = {w: i for i, w in enumerate(what)}
        assert rect_cells(label[0], corners[0]) == 256 and (n < 2 or rect_cells(label[1], corners[1]) == 324)
        # (the rays through the outermost columns and rows meet the front face's edge exactly: t_in == t_out is no hit; 14 x 14 and 16 x 16 remain)
        assert profile[0, mid, 0] == 196 and profile[1, mid, 0] == 256 and not profile[:2, mid, 5].any(), profile[:2, mid]
    if n >= 65:
        assert flags[row['outside the image']] == abi.VIS_NO_RAYS | abi.VIS_NO_EVIDENCE and not profile[row['outside the image']].any()
        assert flags[row['a corner behind the camera']] == abi.VIS_BEHIND and not profile[row['a corner behind the camera'], mid].any()
        assert flags[row['a zero-length edge']] & ~abi.VIS_SNAPPED == 0 and profile[row['a zero-length edge'], mid, 0] > 0
        for w in ('a NaN label', 'an infinite corner'):
            assert flags[row[w]] == abi.VIS_NOT_FINITE and not profile[row[w]].any() and choice[row[w]] == mid
        for w in ('no scene', 'a scene whose grid does not fit'):
            assert flags[row[w]] == abi.VIS_NO_SCENE and not profile[row[w]].any() and not measures[row[w]].any()
        for bit in (abi.VIS_NO_EVIDENCE,) + ((abi.VIS_SNAPPED,) if mode and K > 1 else ()):
            assert (flags & bit).any(), 'no row with flag %d' % bit
        if K == 9:                                             # the tie rules, on rows where they decide
            score = profile[:, :, 3].astype(np.int64) - profile[:, :, 4]
            top = score == score.max(1, keepdims=True)
            tied = (top.sum(1) > 1) & ((flags & FV.REFUSING) == 0)
            dist = np.abs(np.arange(K) - mid)
            nearer = tied & np.array([len(set(dist[t])) > 1 for t in top])
            assert tied.sum() >= 8 and nearer.sum() >= 4, (tied.sum(), nearer.sum())
            for i in np.nonzero(tied)[0]:
                assert dist[choice[i]] == dist[top[i]].min() and choice[i] == min(k for k in np.nonzero(top[i])[0] if dist[k] == dist[choice[i]])
        if K == 3:                                             # equal scores at equal distances either side of the box: the lower k, and too small a gain
            i = row['a tie of the candidates either side']
            assert profile[i, :, 1:5].tolist() == [[1, 0, 2, 1], [1, 2, 0, 1], [1, 2, 1, 0]] and choice[i] == 0 and flags[i] == 0, (profile[i], choice[i], flags[i])
        if mode and K > 1:                                     # min_gain: a better candidate that does not beat the box by enough
            score = profile[:, :, 3].astype(np.int64) - profile[:, :, 4]
            gain = score[np.arange(n), choice] - score[:, mid]
            ok = (flags & FV.REFUSING) == 0
            assert (ok & (choice != mid) & (gain < MIN_GAIN)).any() and not (moved & (gain < MIN_GAIN)).any()
            assert np.array_equal(moved, ok & (choice != mid) & (gain >= MIN_GAIN)) and moved.sum() >= 4
            o = OFFSETS[K][choice[moved]]
            assert same(lo[moved, 3], (label[moved, 3].astype(np.float64) + o * label[moved, 3].astype(np.float64)).astype(np.float32))
    if mode == 0:                                              # measuring needs no output boxes
        again = run_detect_visibility(rt, label, corners, index, cal, dims, goff, range_, OFFSETS[K], 0, outputs=False)
        compare(again[:4], got[:4], 'without output boxes')


def specification(n, K, mode):
    key = (n, K, mode)
    if key not in _SPEC:
        label, corners, index = detections(n)
        cal, dims, goff, range_ = world()
        _SPEC[key] = FV.detect_visibility(label, corners, index, cal, dims, goff, range_, CELL, OFFSETS[K], MARGIN, MIN_CHORD, MIN_GAIN, mode)
    return _SPEC[key]


_SPEC = {}
DETECT_SIZES = (0, 1, 2, 65, 257)


def check_detect_batch_independence(rt):
    """A detection's bytes do not depend on the batch it is measured in."""
    label, corners, index = detections(65)
    cal, dims, goff, range_ = world()
    whole = run_detect_visibility(rt, label, corners, index, cal, dims, goff, range_, OFFSETS[9], 1)
    rows = np.array([64, 3, 17, 0, 40])
    part = run_detect_visibility(rt, label[rows], corners[rows], index[rows], cal, dims, goff, range_, OFFSETS[9], 1)
    for name, w, p in zip(NAMES, whole, part):
        assert same(w[rows], p), name


def check_detect_visibility_refusals(lib):
    null = C.c_void_p(0)
    a = abi.DetectVisibilityArgs()
    a.struct_size -= 8
    assert lib.t3d_detect_visibility(C.byref(a), null) == abi.ERR_ABI
    assert lib.t3d_detect_visibility(None, null) == -1
    buf, ibuf, fbuf = np.zeros(1 << 12), np.zeros(1 << 12, np.int32), np.zeros(1 << 12, np.float32)
    Dp, Ip, Fp = buf.ctypes.data_as(abi.D), ibuf.ctypes.data_as(abi.I), fbuf.ctypes.data_as(abi.F)
    Lp, Up = C.cast(Dp, abi.L), C.cast(Ip, abi.U32)
    offs = lambda *v: (C.c_double * abi.VIS_MAX_OFFSETS)(*v)

    def call(**kw):
        f = dict(n=4, n_scenes=2, mode=1, K=3, cell=4, min_gain=4, reserved=0, label=Fp, corners=Fp, scene_index=Ip, calib=Dp, grid_dims=Ip,
                 grid_offsets=Lp, range=Up, n_cells=64, margin=0.05, min_chord=0.1, offsets=offs(-0.1, 0.0, 0.1), profile=Ip, measures=Dp, choice=Ip,
                 flags=Ip, label_out=Fp, corners_out=Fp)
        f.update(kw)
        return lib.t3d_detect_visibility(C.byref(abi.DetectVisibilityArgs(**f)), null)
    for k in ('label', 'corners', 'label_out', 'corners_out'):
        assert call(**{k: abi.F()}) == -1, k
    for k in ('scene_index', 'grid_dims', 'profile', 'choice', 'flags'):
        assert call(**{k: abi.I()}) == -1, k
    assert call(calib=abi.D()) == -1 and call(measures=abi.D()) == -1 and call(grid_offsets=abi.L()) == -1 and call(range=abi.U32()) == -1
    assert call(reserved=1) == -1 and call(n=-1) == -1 and call(n_scenes=-1) == -1 and call(n_cells=-1) == -1 and call(mode=2) == -1 and call(mode=-1) == -1
    assert call(cell=0) == -1 and call(min_gain=-1) == -1
    for k in ('margin', 'min_chord'):
        for bad in (-0.1, float('nan'), float('inf')):
            assert call(**{k: bad}) == -1, (k, bad)
    assert call(K=0) == -2 and call(K=2) == -2 and call(K=19) == -2 and call(K=-1) == -2
    for bad in (offs(-0.1, 0.0, 0.0), offs(0.1, 0.0, 0.2), offs(-1.0, 0.0, 0.1), offs(-0.1, 0.01, 0.1), offs(-0.1, 0.0, float('nan')), offs(-0.1, 0.0, float('inf'))):
        assert call(offsets=bad) == -1, list(bad)[:3]
    assert call(K=1, offsets=offs(0.5)) == -1 and call(K=1, offsets=offs(0.0), n=0) == 0
    assert call(n=0) == 0 and call(n=0, mode=0, label_out=abi.F(), corners_out=abi.F()) == 0, 'no detection: nothing to do, and nothing is launched'
    assert call(n=0, n_scenes=0, calib=abi.D(), grid_dims=abi.I(), grid_offsets=abi.L(), n_cells=0, range=abi.U32()) == 0
    assert not buf.any() and not ibuf.any() and not fbuf.any()
