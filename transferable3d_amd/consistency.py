"""Label-free consistency of decoded detections on the device (t3d_detect_consistency, csrc/consistency.hip).

A 3-D box that was predicted from a 2-D box can be checked without ground truth: it has to reproject onto its 2-D box, and it has to sit
on the points the network segmented (the two relations the weak losses of csrc/weak.hip train).  `DeviceConsistency` measures both on
finished detections, behind t3d_detect_decode and on the buffers it wrote:

    reproj_iou    IoU of the image rectangle around the eight projected corners (clipped to the image where its size is known) with
                  the 2-D box the frustum was cut from
    mask_in_box   n_both / n_mask: the share of the segmented points that lie inside the 3-D box
    seg_box_iou   n_both / (n_mask + n_box - n_both): IoU of the segmented points with the frustum's points inside the box

The last two are computed here, on the host, from the kernel's integer counts.  `Test` is the form in which this module and the later
stages (ensemble, rescore, floor, visibility) each state the tests that reject a detection by their measure; `log_line` prints them.  Nothing runs this unless it is asked for (detect
--consistency / --min_*, autolabel).
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import abi
from .abi import dptr, fptr, iptr

BAD_PROJECTION, EMPTY_MASK, NO_CALIB = abi.CONSISTENCY_BAD_PROJECTION, abi.CONSISTENCY_EMPTY_MASK, abi.CONSISTENCY_NO_CALIB
THRESHOLDS = ('min_reproj_iou', 'min_mask_in_box', 'min_seg_box_iou')
MEASURES = ('reproj_iou', 'mask_in_box', 'seg_box_iou')

# A test that can reject a detection, stated once beside the stage that takes its measure: the flag that carries its limit; the fields
# it reads (attributes of semisup_infer.Decoded and keys of autolabel's records; visibility_evidence is a record's name for through +
# inside of Decoded.visibility_profile); its fragment of the `consistency:` line; rejected(*fields, limit, **parameters) -> [n] bool; and
# the parameters it takes besides the limit, attributes of the options its stage was given.  semisup_infer.TESTS names them all, in order.
Test = collections.namedtuple('Test', 'flag fields fragment rejected parameters')


def lies_below(values, limit):
    """[n] bool: the value lies below the limit.  A NaN fails the `>=`, so it lies below every limit."""
    return ~(np.asarray(values) >= limit)


TESTS = tuple(Test(flag, (measure,), measure + ' < %g', lies_below, ()) for flag, measure in zip(THRESHOLDS, MEASURES))


def calib_row(Rtilt, K, image_wh=None):
    """One row of the kernel's calibration table: Rtilt row-major (9), K row-major (9), image W, image H (0, 0: do not clip)."""
    w, h = (0.0, 0.0) if image_wh is None else (float(image_wh[0]), float(image_wh[1]))
    return np.concatenate([np.asarray(Rtilt, np.float64).reshape(9), np.asarray(K, np.float64).reshape(9), [w, h]])


def image_size(path):
    """(W, H) of an image file, read from its header (the pixels are not decoded)."""
    from PIL import Image
    with Image.open(path) as im:
        return im.size


def derived(n_mask, n_box, n_both):
    """(mask_in_box, seg_box_iou) fp64 from the integer counts; 0 where a denominator is 0."""
    n_mask, n_box, n_both = (np.asarray(a, np.int64) for a in (n_mask, n_box, n_both))
    union = n_mask + n_box - n_both
    return (np.where(n_mask > 0, n_both / np.maximum(n_mask, 1), 0.0), np.where(union > 0, n_both / np.maximum(union, 1), 0.0))


def check_thresholds(min_reproj_iou=None, min_mask_in_box=None, min_seg_box_iou=None):
    """-> the three thresholds as floats or None; ValueError for one outside [0, 1]."""
    out = []
    for name, v in zip(THRESHOLDS, (min_reproj_iou, min_mask_in_box, min_seg_box_iou)):
        if v is not None:
            v = float(v)
            if not 0.0 <= v <= 1.0:                  # (a NaN fails too)
                raise ValueError('--%s must lie in [0, 1], got %r' % (name, v))
        out.append(v)
    return tuple(out)


def add_arguments(parser):
    parser.add_argument('--consistency', action='store_true',
                        help='measure, per detection, the IoU of its reprojected 3-D box with its 2-D box and how it sits on the segmented points')
    parser.add_argument('--min_reproj_iou', type=float, default=None, help='reject a detection whose reprojection IoU lies below this (0..1)')
    parser.add_argument('--min_mask_in_box', type=float, default=None,
                        help='reject a detection with less than this share of its segmented points inside its 3-D box (0..1)')
    parser.add_argument('--min_seg_box_iou', type=float, default=None,
                        help='reject a detection whose IoU of segmented points and points inside the box lies below this (0..1)')


class ConsistencyRequest:
    """What `semisup_infer.inference(decode='device', consistency=...)` needs per detection: box2d [n, 4] (xmin, ymin, xmax, ymax),
    calib_rows [n_calib, 20] (`calib_row`) and calib_index [n], the row of each detection.  The three thresholds (each or None) make
    `Decoded.accept`; without any, every detection is accepted."""

    def __init__(self, box2d, calib_rows, calib_index, min_reproj_iou=None, min_mask_in_box=None, min_seg_box_iou=None):
        self.box2d = np.ascontiguousarray(box2d, np.float64).reshape(-1, 4)
        self.calib_rows = np.ascontiguousarray(calib_rows, np.float64).reshape(-1, abi.CONSISTENCY_CALIB_WIDTH)
        self.calib_index = np.ascontiguousarray(calib_index, np.int32).reshape(-1)
        if len(self.calib_index) != len(self.box2d):
            raise ValueError('%d 2-D boxes, %d calibration indices' % (len(self.box2d), len(self.calib_index)))
        self.thresholds = check_thresholds(min_reproj_iou, min_mask_in_box, min_seg_box_iou)
        self.min_reproj_iou, self.min_mask_in_box, self.min_seg_box_iou = self.thresholds

    def __len__(self):
        return len(self.box2d)


def accept_of(reproj_iou, mask_in_box, seg_box_iou, thresholds):
    """-> (accept [n] bool, {threshold name: how many detections lie below it}).  A detection below any threshold given is rejected."""
    accept = np.ones(len(reproj_iou), bool)
    counts = {}
    for test, v, t in zip(TESTS, (reproj_iou, mask_in_box, seg_box_iou), thresholds):
        if t is not None:
            bad = test.rejected(v, t)
            counts[test.flag] = int(bad.sum())
            accept &= ~bad
    return accept, counts


def log_line(accept, below, thresholds, tests=TESTS):
    """The `consistency:` line: how many of `accept` are True and, per test with a limit (`thresholds` runs beside `tests`), its
    fragment with below[its flag], the number of detections it rejects."""
    parts = [(t.fragment + ': %d') % (limit, below[t.flag]) for t, limit in zip(tests, thresholds) if limit is not None]
    return 'consistency: kept %d of %d (%s)' % (int(np.sum(accept)), len(accept), ', '.join(parts) if parts else 'no threshold')


class DeviceConsistency:
    """Output buffers of t3d_detect_consistency for `n` detections of `num_point` points each, the per-detection inputs of a request on
    the device, and the launch of one batch."""

    def __init__(self, rt, n, num_point, request=None):
        self.rt, self.n, self.N = rt, n, num_point
        self.counts = rt.zeros(n, 4, dtype=torch.int32)
        self.reproj = rt.zeros(n, 5, dtype=torch.float64)
        self.box2d = self.calib = self.calib_index = None
        self.n_calib = 0
        self.thresholds = (None, None, None)
        if request is not None:
            self.upload(request)

    def upload(self, req):
        """The request's rows 0 .. len(req)-1 are detections 0 .. of the outputs; the rows past them (the padding of a last batch) name no
        calibration row."""
        if len(req) > self.n:
            raise ValueError('%d detections in the request, room for %d' % (len(req), self.n))
        box2d, index = np.zeros((self.n, 4)), np.full(self.n, -1, np.int32)
        box2d[:len(req)], index[:len(req)] = req.box2d, req.calib_index
        dev = self.rt.device
        self.box2d, self.calib_index = torch.from_numpy(box2d).to(dev), torch.from_numpy(index).to(dev)
        rows = req.calib_rows if len(req.calib_rows) else np.zeros((1, abi.CONSISTENCY_CALIB_WIDTH))
        self.calib, self.n_calib = torch.from_numpy(rows).to(dev), len(req.calib_rows)
        self.thresholds = req.thresholds

    def launch(self, first, B, n_valid, xyz, ld_xyz, logits, corners, rot_angle=None):
        """Measure the batch whose detections are rows first .. first + B - 1 of the outputs; the first `n_valid` of them are real.
        xyz: the [B * N, ld_xyz] fp32 points the network read; logits [B, N, 2]; corners: rows first .. of what t3d_detect_decode wrote."""
        assert 0 <= first and first + B <= self.n and logits.numel() == B * self.N * 2 and xyz.numel() >= B * self.N * int(ld_xyz)
        assert xyz.dtype == torch.float32 and logits.dtype == torch.float32 and corners.dtype == torch.float32 and corners.is_contiguous()
        a = abi.DetectConsistencyArgs(B, self.N, int(n_valid), int(ld_xyz), fptr(xyz), fptr(logits), fptr(corners), fptr(rot_angle),
                                      dptr(self.box2d[first:]), iptr(self.calib_index[first:]), dptr(self.calib), self.n_calib,
                                      iptr(self.counts[first:]), dptr(self.reproj[first:]))
        abi.check(self.rt.lib.t3d_detect_consistency(C.byref(a), self.rt.stream()), 't3d_detect_consistency')

    def fetch(self):
        """-> dict of host arrays, one row per detection: reproj_rect [n, 4], reproj_iou, n_mask, n_box, n_both, flags, mask_in_box,
        seg_box_iou, accept (bool: no threshold of the request is missed).  The one small copy back."""
        counts, reproj = self.counts.cpu().numpy().astype(np.int64), self.reproj.cpu().numpy()
        out = dict(reproj_rect=reproj[:, :4].copy(), reproj_iou=reproj[:, 4].copy(), n_mask=counts[:, 0], n_box=counts[:, 1],
                   n_both=counts[:, 2], flags=counts[:, 3])
        out['mask_in_box'], out['seg_box_iou'] = derived(out['n_mask'], out['n_box'], out['n_both'])
        out['accept'], out['below'] = accept_of(out['reproj_iou'], out['mask_in_box'], out['seg_box_iou'], self.thresholds)
        return out
