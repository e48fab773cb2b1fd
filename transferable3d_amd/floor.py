"""The floor of a scene, fitted on the device, and the detections standing on it (t3d_scene_floor, t3d_detect_floor, csrc/floor.hip).

Every label-free measure of a detection so far looks inside the frustum the box came from.  The scene knows one thing the frustum seldom
shows: all evaluated classes stand on the floor.  `DeviceFloor` estimates the floor plane of every scene of an extraction launch from
the depth points the launch left on the device (the lowest peak of a height histogram that holds enough of the points, then a plane
through the points around it); `DeviceFloorStage` measures, behind the decode, how far the bottom of every box lies from that plane
(`floor_gap`: positive, the box floats; negative, it sinks) and on request stands the box on it -- 'shift' moves the box, 'stretch'
moves its bottom face and keeps the top.  Nothing runs this unless it is asked for (detect --floor / --snap_floor / --max_floor_gap).
"""
import ctypes as C
import json
import math

import numpy as np
import torch

from . import abi
from .abi import dptr, fptr, iptr
from .consistency import Test

NONE, LEVEL = abi.FLOOR_NONE, abi.FLOOR_LEVEL
NO_FLOOR, NOT_FINITE, TOO_FAR, INVERTED, SNAPPED = (abi.DETECT_FLOOR_NO_FLOOR, abi.DETECT_FLOOR_NOT_FINITE, abi.DETECT_FLOOR_TOO_FAR,
                                                    abi.DETECT_FLOOR_INVERTED, abi.DETECT_FLOOR_SNAPPED)
UNKNOWN = NO_FLOOR | NOT_FINITE                   # the gap of such a detection is NaN: it is neither snapped nor rejected
MODES = {None: 0, 'shift': 1, 'stretch': 2}
SNAP_MAX = 0.3
ESTIMATOR_FLAGS = ('floor_bin', 'floor_range', 'floor_min_share', 'floor_band', 'floor_max_tilt')
FLAGS = ('floor', 'snap_floor', 'snap_floor_max', 'max_floor_gap') + ESTIMATOR_FLAGS


class FloorOptions:
    """The options of the estimator, checked: bin (m) and range (z_lo, z_hi: heights of the depth frame, camera at 0) of the height
    histogram, min_share (of the finite points) and min_inliers a peak must hold, band (m) around the peak's centre whose points the
    plane is fitted to, max_tilt (degrees) of an accepted plane, min_spread (m, rms extent of the inliers along X and along Y) and
    min_det_ratio (1 - correlation^2 of their X and Y) below which the floor is taken as level."""

    def __init__(self, bin=0.02, range=(-3.0, -0.2), min_share=0.02, min_inliers=50, band=0.05, max_tilt=5.0, min_spread=0.25,
                 min_det_ratio=0.05):
        self.bin, self.z_lo, self.z_hi = float(bin), float(range[0]), float(range[1])
        self.min_share, self.min_inliers, self.band = float(min_share), int(min_inliers), float(band)
        self.max_tilt, self.min_spread, self.min_det_ratio = float(max_tilt), float(min_spread), float(min_det_ratio)
        if not (0.0 < self.bin < math.inf):
            raise ValueError('--floor_bin must be a finite number above 0, got %r' % self.bin)
        if not (self.z_lo < self.z_hi and math.isfinite(self.z_lo) and math.isfinite(self.z_hi)):
            raise ValueError('--floor_range LO HI needs finite LO < HI, got %r %r' % (self.z_lo, self.z_hi))
        if not 0.0 <= self.min_share <= 1.0:
            raise ValueError('--floor_min_share must lie in [0, 1], got %r' % self.min_share)
        if not (0.0 <= self.band < math.inf):
            raise ValueError('--floor_band must be a finite number, not negative, got %r' % self.band)
        if not 0.0 <= self.max_tilt < 90.0:
            raise ValueError('--floor_max_tilt must lie in [0, 90) degrees, got %r' % self.max_tilt)
        if self.min_inliers < 0 or not self.min_spread >= 0.0 or not self.min_det_ratio >= 0.0:
            raise ValueError('min_inliers, min_spread and min_det_ratio must not be negative')
        self.n_bins = int(math.ceil((self.z_hi - self.z_lo) / self.bin - 1e-9))
        if not 1 <= self.n_bins <= abi.SCENE_FLOOR_MAX_BINS:
            raise ValueError('--floor_range / --floor_bin: %d bins, at most %d' % (self.n_bins, abi.SCENE_FLOOR_MAX_BINS))
        self.inv_bin = 1.0 / self.bin
        self.max_slope2 = math.tan(math.radians(self.max_tilt)) ** 2

    def kernel_options(self):
        """The options as t3d_scene_floor's argument struct names them."""
        return dict(z_lo=self.z_lo, z_hi=self.z_hi, bin=self.bin, inv_bin=self.inv_bin, n_bins=self.n_bins, min_share=self.min_share,
                    min_inliers=self.min_inliers, band=self.band, max_slope2=self.max_slope2, min_spread=self.min_spread,
                    min_det_ratio=self.min_det_ratio)


def _number(name, v, lo_open=False):
    v = float(v)
    if not (v > 0.0 if lo_open else v >= 0.0) or not math.isfinite(v):
        raise ValueError('--%s must be a finite number %s, got %r' % (name, 'above 0' if lo_open else 'that is not negative', v))
    return v


class Floor:
    """The checked options of the stage as `Detector` holds them: on, snap (None / 'shift' / 'stretch'), snap_max, max_floor_gap (or
    None), options (FloorOptions)."""

    def __init__(self, on, snap, snap_max, max_floor_gap, options):
        self.on, self.snap, self.snap_max, self.max_floor_gap, self.options = on, snap, snap_max, max_floor_gap, options


def check_options(floor=False, snap_floor=None, snap_floor_max=None, max_floor_gap=None, floor_bin=None, floor_range=None,
                  floor_min_share=None, floor_band=None, floor_max_tilt=None):
    """-> Floor; ValueError for an option without the flag it belongs to and for a value no flag takes."""
    if snap_floor not in MODES:
        raise ValueError("--snap_floor is 'shift' or 'stretch', got %r" % (snap_floor,))
    if snap_floor_max is not None and snap_floor is None:
        raise ValueError('--snap_floor_max bounds the move of --snap_floor: it needs --snap_floor')
    snap_max = SNAP_MAX if snap_floor_max is None else _number('snap_floor_max', snap_floor_max)
    gap = None if max_floor_gap is None else _number('max_floor_gap', max_floor_gap)
    on = bool(floor) or snap_floor is not None or gap is not None
    given = {'floor_bin': floor_bin, 'floor_range': floor_range, 'floor_min_share': floor_min_share, 'floor_band': floor_band,
             'floor_max_tilt': floor_max_tilt}
    given = {k: v for k, v in given.items() if v is not None}
    if given and not on:
        raise ValueError('%s set%s the floor estimator: %s --floor, --snap_floor or --max_floor_gap'
                         % (' '.join('--' + k for k in given), 's' if len(given) == 1 else '', 'it needs' if len(given) == 1 else 'they need'))
    kw = {k[len('floor_'):]: v for k, v in given.items()}
    return Floor(on, snap_floor, snap_max, gap, FloorOptions(**kw))


def add_arguments(parser):
    parser.add_argument('--floor', action='store_true', help='fit every scene\'s floor plane on the device and measure each box\'s floor_gap')
    parser.add_argument('--snap_floor', choices=['shift', 'stretch'], default=None,
                        help='stand every box on its scene\'s floor: shift moves the box, stretch moves its bottom and keeps its top (implies --floor)')
    parser.add_argument('--snap_floor_max', type=float, default=None, help='--snap_floor: leave a box whose |floor_gap| exceeds this (m; default %g)' % SNAP_MAX)
    parser.add_argument('--max_floor_gap', type=float, default=None, help='reject a detection whose |floor_gap| exceeds this (m; implies --floor)')
    parser.add_argument('--floor_bin', type=float, default=None, help='bin of the height histogram (m; default 0.02)')
    parser.add_argument('--floor_range', type=float, nargs=2, default=None, metavar=('LO', 'HI'), help='heights searched for the floor, camera at 0 (m; default -3.0 -0.2)')
    parser.add_argument('--floor_min_share', type=float, default=None, help='share of a scene\'s points the floor peak must hold (default 0.02)')
    parser.add_argument('--floor_band', type=float, default=None, help='half-width around the peak of the points the plane is fitted to (m; default 0.05)')
    parser.add_argument('--floor_max_tilt', type=float, default=None, help='largest tilt of an accepted plane (degrees; default 5)')


class DeviceFloor:
    """t3d_scene_floor on the points of an extraction launch."""

    def __init__(self, rt, options=None):
        self.rt, self.options = rt, options if options is not None else FloorOptions()
        self.hist = None

    def estimate(self, points, scene_offsets):
        """points [sum n_s, ld >= 3] fp64 on the device (upright depth coordinates), scene_offsets [S + 1] (host or device) -> (plane
        [S, 8] fp64 and counts [S, 4] int32 on the device, counts on the host: the one small copy back).  `hist` [S, n_bins] stays here."""
        o, dev = self.options, self.rt.device
        offsets = torch.as_tensor(np.ascontiguousarray(scene_offsets) if isinstance(scene_offsets, np.ndarray) else scene_offsets).to(torch.int64).to(dev).contiguous()
        S = int(offsets.numel()) - 1
        assert S >= 0 and points.dtype == torch.float64 and points.dim() == 2 and points.stride(1) == 1 and points.shape[1] >= 3
        plane = torch.zeros(max(S, 1), 8, dtype=torch.float64, device=dev)
        counts = torch.zeros(max(S, 1), 4, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(max(S, 1), o.n_bins, dtype=torch.int32, device=dev)
        work = torch.zeros(max(abi.scene_floor_workspace_bytes(S) // 8, 1), dtype=torch.int64, device=dev)
        a = abi.SceneFloorArgs(S, int(points.stride(0)), o.n_bins, dptr(points), C.cast(C.c_void_p(offsets.data_ptr()), abi.L), o.z_lo, o.z_hi,
                               o.bin, o.inv_bin, o.min_share, o.min_inliers, 0, o.band, o.max_slope2, o.min_spread, o.min_det_ratio,
                               C.c_void_p(work.data_ptr()), work.numel() * 8, dptr(plane), iptr(counts), iptr(self.hist))
        abi.check(self.rt.lib.t3d_scene_floor(C.byref(a), self.rt.stream()), 't3d_scene_floor')
        return plane[:S], counts[:S], counts[:S].cpu().numpy()


class FloorRequest:
    """What `semisup_infer.inference(decode='device', floor=...)` needs: planes [S, 8] and counts [S, 4] as t3d_scene_floor wrote them
    (device tensors or arrays), scene_index [n] the row of each detection (-1: none), snap (None: measure only), snap_max (a box
    further than this from the floor is left alone) and max_floor_gap (None, or the |floor_gap| above which a detection is rejected)."""

    def __init__(self, planes, counts, scene_index, snap=None, snap_max=SNAP_MAX, max_floor_gap=None):
        if snap not in MODES:
            raise ValueError("snap is None, 'shift' or 'stretch', got %r" % (snap,))
        self.planes, self.counts = planes, counts
        self.scene_index = np.ascontiguousarray(scene_index, np.int32).reshape(-1)
        if tuple(planes.shape[1:]) != (8,) or tuple(counts.shape[1:]) != (4,) or len(planes) != len(counts):
            raise ValueError('planes [S, 8] and counts [S, 4] of the same scenes, got %s and %s' % (tuple(planes.shape), tuple(counts.shape)))
        if len(self.scene_index) and (self.scene_index.min() < -1 or self.scene_index.max() >= len(planes)):
            raise ValueError('a scene index outside -1 .. %d' % (len(planes) - 1))
        self.snap, self.snap_max = snap, _number('snap_floor_max', snap_max)
        self.max_floor_gap = None if max_floor_gap is None else _number('max_floor_gap', max_floor_gap)

    def __len__(self):
        return len(self.scene_index)

    def counts_host(self):
        c = self.counts
        return np.asarray(c.cpu().numpy() if isinstance(c, torch.Tensor) else c, np.int64).reshape(-1, 4)


class DeviceFloorStage:
    """The buffers and the launch of t3d_detect_floor."""

    def __init__(self, rt):
        self.rt = rt
        self.gap = self.flags = self.label_out = self.corners_out = None

    def run(self, label, corners, request, n=None):
        """label [n, 7], corners [n, 24] fp32 on the device; the request's rows are detections 0 .. len(request) - 1, the rows past them
        (the padding of a last batch) have no scene.  -> (label_out, corners_out) where the request snaps, else None; `gap` [n] fp64 and
        `flags` [n] int32 stay on the device."""
        rt, dev = self.rt, self.rt.device
        n = int(label.shape[0]) if n is None else int(n)
        if len(request) > n:
            raise ValueError('%d detections in the floor request, room for %d' % (len(request), n))
        assert label.dtype == torch.float32 and corners.dtype == torch.float32 and label.is_contiguous() and corners.is_contiguous()
        index = np.full(n, -1, np.int32)
        index[:len(request)] = request.scene_index
        index = torch.from_numpy(index).to(dev)
        up = lambda t, dt: (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).to(dt).to(dev).contiguous()
        planes, counts = up(request.planes, torch.float64), up(request.counts, torch.int32)
        S = int(planes.shape[0])
        self.gap = abi.grown(self.gap, n, torch.float64, dev)
        self.flags = abi.grown(self.flags, n, torch.int32, dev)
        mode = MODES[request.snap]
        if mode:
            self.label_out = abi.grown(self.label_out, n, torch.float32, dev, 7)
            self.corners_out = abi.grown(self.corners_out, n, torch.float32, dev, 24)
        a = abi.DetectFloorArgs(n, S, mode, fptr(label), fptr(corners), iptr(index), dptr(planes if S else None), iptr(counts if S else None),
                                request.snap_max, 0, dptr(self.gap), iptr(self.flags), fptr(self.label_out if mode else None),
                                fptr(self.corners_out if mode else None))
        abi.check(rt.lib.t3d_detect_floor(C.byref(a), rt.stream()), 't3d_detect_floor')
        return (self.label_out[:n], self.corners_out[:n]) if mode else None


def rejected(gap, flags, max_floor_gap):
    """[n] bool: the floor is known and |gap| > max_floor_gap (the gap measured before any snapping; a NaN exceeds nothing)."""
    with np.errstate(invalid='ignore'):
        return ((np.asarray(flags, np.int64) & UNKNOWN) == 0) & (np.abs(gap) > max_floor_gap)


TEST = Test('max_floor_gap', ('floor_gap', 'floor_flags'), '|floor_gap| > %g', rejected, ())       # the stage's rejecting test (consistency.Test)


def log_line(request, gap, flags):
    """The `floor:` line of a run: gap, flags of its real detections."""
    c = request.counts_host()
    with_floor = (c[:, 3] & NONE) == 0
    known = (np.asarray(flags) & UNKNOWN) == 0
    g = np.asarray(gap)[known]
    med, med_abs = (float(np.median(g)), float(np.median(np.abs(g)))) if len(g) else (float('nan'), float('nan'))
    line = 'floor: %d of %d scenes with a floor (level only: %d), median gap %+.2f m (abs %.2f)' % (
        int(with_floor.sum()), len(c), int((with_floor & ((c[:, 3] & LEVEL) != 0)).sum()), med, med_abs)
    if request.snap is not None:
        line += ', snapped %d of %d boxes (%s, |gap| <= %g)' % (int(((np.asarray(flags) & SNAPPED) != 0).sum()), len(flags), request.snap, request.snap_max)
    if request.max_floor_gap is not None:
        line += ', rejected %d (|gap| > %g)' % (int(rejected(gap, flags, request.max_floor_gap).sum()), request.max_floor_gap)
    return line


def scene_rows(ids, plane, counts):
    """--floor_json: per scene its id, plane (a, b, c), the inliers' centroid, their share of the finite points, the rms distance of
    the inliers from the plane and the flags."""
    rows = []
    for i, p, c in zip(ids, np.asarray(plane, np.float64), np.asarray(counts, np.int64)):
        rows.append({'scene': int(i), 'plane': [float(v) for v in p[:3]], 'centroid': [float(v) for v in p[3:6]], 'peak': float(p[7]),
                     'n_finite': int(c[0]), 'n_inliers': int(c[1]), 'share': float(c[1]) / float(c[0]) if c[0] > 0 else 0.0,
                     'rms': math.sqrt(float(p[6])), 'flags': int(c[3]), 'floor': not (int(c[3]) & NONE), 'level_only': bool(int(c[3]) & LEVEL)})
    return rows


def write_json(path, rows):
    with open(path, 'w') as fh:
        json.dump(rows, fh, indent=1)
