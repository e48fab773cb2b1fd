"""Every box against the free space of its scene, on the device (t3d_scene_range, t3d_detect_visibility, csrc/range.hip).

A depth image says of every pixel that the space between the camera and its return is empty.  A box pulled towards the camera has the
wall behind it visible THROUGH it, a box pushed away has every return IN FRONT of it, a background box in mid-air is seen through
entirely.  `DeviceRange` keeps that fact of every scene of an extraction launch as a range map -- per cell of `cell` x `cell` pixels the
nearest return, the conservative choice: a cell that straddles an object's edge reports the foreground, so it can never claim that a box
is seen through -- built from the depth points the launch left on the device; a few KB per scene stay, the points go.
`DeviceVisibilityStage` casts, behind the decode, a ray through every cell a box covers and counts where the cell's return lies: in
front of the box, inside it, or behind it (`see_through`, `occluded`, `support`).  Nothing runs this unless it is asked for (detect
--visibility / --max_see_through).

The kernel can also compare a box with copies of it slid along its viewing ray and move it to the best one (t3d.h: candidates, mode 1).
No command offers that: on clean label boxes of generated scenes the rule brought back fewer than half of the boxes displaced by two
steps, for every seed tried (README) -- a box pulled towards the camera still holds its object's visible front, so its score hardly
changes.  The stage here measures the box as it stands.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import abi
from .abi import dptr, fptr, iptr
from .consistency import Test, calib_row

NO_SCENE, NOT_FINITE, BEHIND, NO_RAYS, NO_EVIDENCE = abi.VIS_NO_SCENE, abi.VIS_NOT_FINITE, abi.VIS_BEHIND, abi.VIS_NO_RAYS, abi.VIS_NO_EVIDENCE
UNMEASURED = NO_SCENE | NOT_FINITE | BEHIND        # such a detection is not rejected
RAYS, UNKNOWN, FRONT, INSIDE, THROUGH, GRAZE = range(6)      # abi.VIS_PROFILE
FLAGS = ('visibility', 'visibility_cell', 'visibility_margin', 'visibility_min_chord', 'max_see_through', 'visibility_min_rays')
DEFAULTS = dict(cell=4, margin=0.05, min_chord=0.1, min_rays=16)      # options, not tuned values


class VisibilityOptions:
    """The options of the two kernels, checked: cell (pixels a side of a cell of the range map), margin (m: a return this far in front
    of or behind the box still counts as inside), min_chord (m: a ray that crosses less of the box is a graze) and min_rays (through +
    inside a detection needs for --max_see_through to reject it)."""

    def __init__(self, cell=DEFAULTS['cell'], margin=DEFAULTS['margin'], min_chord=DEFAULTS['min_chord'], min_rays=DEFAULTS['min_rays']):
        if int(cell) != cell or not 1 <= int(cell) <= 1024:
            raise ValueError('--visibility_cell must be a whole number of pixels in [1, 1024], got %r' % (cell,))
        self.cell = int(cell)
        self.margin, self.min_chord = _number('visibility_margin', margin), _number('visibility_min_chord', min_chord)
        if int(min_rays) != min_rays or int(min_rays) < 0:
            raise ValueError('--visibility_min_rays must be a whole number that is not negative, got %r' % (min_rays,))
        self.min_rays = int(min_rays)


def _number(name, v):
    v = float(v)
    if not v >= 0.0 or not math.isfinite(v):
        raise ValueError('--%s must be a finite number that is not negative, got %r' % (name, v))
    return v


class Visibility:
    """The checked options of the stage as `Detector` holds them: on, max_see_through (or None), options (VisibilityOptions)."""

    def __init__(self, on, max_see_through, options):
        self.on, self.max_see_through, self.options = on, max_see_through, options


def check_options(visibility=False, visibility_cell=None, visibility_margin=None, visibility_min_chord=None, max_see_through=None,
                  visibility_min_rays=None):
    """-> Visibility; ValueError for an option without the flag it belongs to and for a value no flag takes."""
    limit = None
    if max_see_through is not None:
        limit = float(max_see_through)
        if not 0.0 <= limit <= 1.0:
            raise ValueError('--max_see_through must lie in [0, 1], got %r' % (max_see_through,))
    on = bool(visibility) or limit is not None
    given = [k for k, v in (('visibility_cell', visibility_cell), ('visibility_margin', visibility_margin), ('visibility_min_chord', visibility_min_chord))
             if v is not None]
    if given and not on:
        raise ValueError('%s set%s the visibility stage: %s --visibility or --max_see_through'
                         % (' '.join('--' + k for k in given), 's' if len(given) == 1 else '', 'it needs' if len(given) == 1 else 'they need'))
    if visibility_min_rays is not None and limit is None:
        raise ValueError('--visibility_min_rays is the evidence --max_see_through asks for before it rejects: it needs --max_see_through')
    kw = dict(cell=visibility_cell, margin=visibility_margin, min_chord=visibility_min_chord, min_rays=visibility_min_rays)
    return Visibility(on, limit, VisibilityOptions(**{k: v for k, v in kw.items() if v is not None}))


def add_arguments(parser):
    d = DEFAULTS
    parser.add_argument('--visibility', action='store_true', help='keep a range map of every scene on the device and measure each box against it: see_through, occluded, support')
    parser.add_argument('--visibility_cell', type=int, default=None, help='side of a cell of the range map (pixels; default %d)' % d['cell'])
    parser.add_argument('--visibility_margin', type=float, default=None, help='a return this far in front of or behind a box still counts as inside (m; default %g)' % d['margin'])
    parser.add_argument('--visibility_min_chord', type=float, default=None, help='a ray that crosses less of the box than this is a graze and counts nowhere (m; default %g)' % d['min_chord'])
    parser.add_argument('--max_see_through', type=float, default=None, metavar='F',
                        help='reject a detection whose see_through exceeds F in [0, 1] on at least --visibility_min_rays rays (implies --visibility)')
    parser.add_argument('--visibility_min_rays', type=int, default=None, help='--max_see_through: the rays behind or inside a box it asks for (default %d)' % d['min_rays'])


def scene_size(scene):
    """(W, H) of a scene's image: its 'image_wh' where known, else twice the principal point, rounded up."""
    wh = scene.get('image_wh')
    if wh is not None:
        return int(wh[0]), int(wh[1])
    K = np.asarray(scene['K'], np.float64).reshape(3, 3)
    return int(math.ceil(2.0 * K[0, 2])), int(math.ceil(2.0 * K[1, 2]))


def grids_of(sizes, cell):
    """The grids of images of `sizes` [(W, H)] -> (grid_dims [S, 2] int32: ceil(W / cell), ceil(H / cell); grid_offsets [S + 1] int64)."""
    dims = np.array([[-(-max(int(w), 0) // cell), -(-max(int(h), 0) // cell)] for w, h in sizes], np.int32).reshape(-1, 2)
    return dims, np.concatenate([[0], np.cumsum(dims[:, 0].astype(np.int64) * dims[:, 1])]).astype(np.int64)


class DeviceRange:
    """t3d_scene_range on the points of an extraction launch."""

    def __init__(self, rt, options=None):
        self.rt, self.options = rt, options if options is not None else VisibilityOptions()

    def build(self, points, scene_offsets, scenes):
        """points [sum n_s, ld >= 3] fp64 on the device (upright depth coordinates), scene_offsets [S + 1] (host or device), scenes:
        [{'Rtilt', 'K', 'image_wh' where known}] -> what a part keeps of its scenes: {'range' [n_cells] int32 on the device (the bits of
        the fp32 depths), 'counts' [S, 4] on the host (the one small copy back), 'calib' [S, 20], 'dims' [S, 2] and 'offsets' [S + 1] on
        the host}."""
        dev, cell = self.rt.device, self.options.cell
        offsets = torch.as_tensor(np.ascontiguousarray(scene_offsets) if isinstance(scene_offsets, np.ndarray) else scene_offsets).to(torch.int64).to(dev).contiguous()
        S = int(offsets.numel()) - 1
        assert S == len(scenes) and points.dtype == torch.float64 and points.dim() == 2 and points.stride(1) == 1 and points.shape[1] >= 3
        calib = np.stack([calib_row(sc['Rtilt'], sc['K'], sc.get('image_wh')) for sc in scenes]) if S else np.zeros((0, 20))
        dims, goff = grids_of([scene_size(sc) for sc in scenes], cell)
        n_cells = int(goff[-1])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        calib_d, dims_d, goff_d = up(calib if S else np.zeros((1, 20))), up(dims if S else np.zeros((1, 2), np.int32)), up(goff)
        index = torch.arange(max(S, 1), dtype=torch.int32, device=dev)
        out = torch.zeros(max(n_cells, 1), dtype=torch.int32, device=dev)
        counts = torch.zeros(max(S, 1), 4, dtype=torch.int32, device=dev)
        a = abi.SceneRangeArgs(S, int(points.stride(0)), cell, S, dptr(points), C.cast(C.c_void_p(offsets.data_ptr()), abi.L), dptr(calib_d),
                               iptr(index), iptr(dims_d), C.cast(C.c_void_p(goff_d.data_ptr()), abi.L), n_cells, 0,
                               C.cast(C.c_void_p(out.data_ptr()), abi.U32), iptr(counts))
        abi.check(self.rt.lib.t3d_scene_range(C.byref(a), self.rt.stream()), 't3d_scene_range')
        return dict(range=out[:n_cells], counts=counts[:S].cpu().numpy(), calib=calib, dims=dims, offsets=goff)


class VisibilityRequest:
    """What `semisup_infer.inference(decode='device', visibility=...)` needs: the scenes' calibration rows [S, 20], grids (grid_dims
    [S, 2], grid_offsets [S + 1]) and range maps (range [n_cells] int32 on the device or an array) as t3d_scene_range took and wrote them,
    scene_index [n] the scene of each detection (-1: none), options (VisibilityOptions) and max_see_through (None, or the see_through
    above which a detection with options.min_rays rays is rejected)."""

    def __init__(self, calib, grid_dims, grid_offsets, range_, scene_index, options=None, max_see_through=None):
        self.calib = np.ascontiguousarray(calib, np.float64).reshape(-1, 20)
        self.grid_dims = np.ascontiguousarray(grid_dims, np.int32).reshape(-1, 2)
        self.grid_offsets = np.ascontiguousarray(grid_offsets, np.int64).reshape(-1)
        self.range = range_
        self.scene_index = np.ascontiguousarray(scene_index, np.int32).reshape(-1)
        S = len(self.calib)
        if len(self.grid_dims) != S or len(self.grid_offsets) != S + 1:
            raise ValueError('calib [S, 20], grid_dims [S, 2] and grid_offsets [S + 1] of the same scenes, got %d, %d and %d rows'
                             % (S, len(self.grid_dims), len(self.grid_offsets)))
        if len(self.scene_index) and (self.scene_index.min() < -1 or self.scene_index.max() >= S):
            raise ValueError('a scene index outside -1 .. %d' % (S - 1))
        self.options = options if options is not None else VisibilityOptions()
        self.max_see_through = None if max_see_through is None else float(max_see_through)
        if self.max_see_through is not None and not 0.0 <= self.max_see_through <= 1.0:
            raise ValueError('max_see_through must lie in [0, 1], got %r' % (max_see_through,))

    def __len__(self):
        return len(self.scene_index)


class DeviceVisibilityStage:
    """The buffers and the launch of t3d_detect_visibility: mode 0 on the box alone (one candidate, offset 0)."""

    def __init__(self, rt):
        self.rt = rt
        self.profile = self.measures = self.choice = self.flags = None

    def run(self, label, corners, request, n=None):
        """label [n, 7], corners [n, 24] fp32 on the device; the request's rows are detections 0 .. len(request) - 1, the rows past them
        (the padding of a last batch) have no scene.  `profile` [n, 6] int32 (abi.VIS_PROFILE), `measures` [n, 3] fp64 and `flags` [n] int32
        stay on the device."""
        rt, dev, o = self.rt, self.rt.device, request.options
        n = int(label.shape[0]) if n is None else int(n)
        if len(request) > n:
            raise ValueError('%d detections in the visibility request, room for %d' % (len(request), n))
        assert label.dtype == torch.float32 and corners.dtype == torch.float32 and label.is_contiguous() and corners.is_contiguous()
        index = np.full(n, -1, np.int32)
        index[:len(request)] = request.scene_index
        up = lambda t, dt: (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).to(dt).to(dev).contiguous()
        index = up(index, torch.int32)
        S = len(request.calib)
        calib, dims, goff = up(request.calib, torch.float64), up(request.grid_dims, torch.int32), up(request.grid_offsets, torch.int64)
        range_ = request.range
        if not isinstance(range_, torch.Tensor):
            range_ = torch.from_numpy(np.ascontiguousarray(range_).view(np.int32))
        range_ = range_.to(dev).contiguous()
        n_cells = int(range_.numel())
        self.profile = abi.grown(self.profile, n, torch.int32, dev, 6)
        self.measures = abi.grown(self.measures, n, torch.float64, dev, 3)
        self.choice = abi.grown(self.choice, n, torch.int32, dev)
        self.flags = abi.grown(self.flags, n, torch.int32, dev)
        offsets = (C.c_double * abi.VIS_MAX_OFFSETS)(0.0)
        a = abi.DetectVisibilityArgs(n, S, 0, 1, o.cell, 0, 0, fptr(label), fptr(corners), iptr(index), dptr(calib if S else None),
                                     iptr(dims if S else None), C.cast(C.c_void_p(goff.data_ptr() if S else 0), abi.L),
                                     C.cast(C.c_void_p(range_.data_ptr() if n_cells else 0), abi.U32), n_cells, o.margin, o.min_chord, offsets,
                                     iptr(self.profile), dptr(self.measures), iptr(self.choice), iptr(self.flags), fptr(None), fptr(None))
        abi.check(rt.lib.t3d_detect_visibility(C.byref(a), rt.stream()), 't3d_detect_visibility')

    def fetch(self, n):
        """-> the host copies of the first n rows: {'profile' [n, 6], 'measures' [n, 3], 'flags' [n]} (int64 / fp64)."""
        return dict(profile=self.profile[:n].cpu().numpy().astype(np.int64), measures=self.measures[:n].cpu().numpy(),
                    flags=self.flags[:n].cpu().numpy().astype(np.int64))


def evidence(profile):
    """through + inside of profile [..., 6]: the rays that say whether a box is seen through ('visibility_evidence' in autolabel's records)."""
    return np.asarray(profile)[..., THROUGH] + np.asarray(profile)[..., INSIDE]


def rejected(see_through, evidence, flags, max_see_through, min_rays):
    """[n] bool: the detection was measured, evidence (through + inside) >= min_rays and see_through > max_see_through."""
    return ((np.asarray(flags, np.int64) & UNMEASURED) == 0) & (np.asarray(evidence) >= min_rays) & (np.asarray(see_through) > max_see_through)


# the stage's rejecting test (consistency.Test); min_rays is VisibilityOptions.min_rays
TEST = Test('max_see_through', ('see_through', 'visibility_evidence', 'visibility_flags'), 'see_through > %g', rejected, ('min_rays',))


def log_line(request, host, n_scenes=None):
    """The `visibility:` line of a run: host = DeviceVisibilityStage.fetch of its real detections."""
    flags = host['flags']
    known = (flags & UNMEASURED) == 0
    see = host['measures'][known, 0]
    line = 'visibility: %d scenes, median see_through %.2f' % (len(request.calib) if n_scenes is None else n_scenes,
                                                               float(np.median(see)) if len(see) else float('nan'))
    if request.max_see_through is not None:
        line += ', rejected %d' % int(rejected(host['measures'][:, 0], evidence(host['profile']), flags, request.max_see_through, request.options.min_rays).sum())
    return line
