"""Test-time augmentation of `detect`: K views per frustum, one fused box and an agreement number (t3d_detect_ensemble, csrc/ensemble.hip).

`detect` sends a frustum through the network once, on one random draw of its points.  With --tta K it goes through K times: view 0 is
that run, view v redraws the points with a seed derived from (seed, v), and with --tta_flip the odd views are mirrored in the frustum's
centre view by t3d_batch_assemble.  t3d_detect_decode writes a label row per view; `DeviceEnsemble.run` follows the last decode with
one call that brings the mirrored boxes back, measures how far the K boxes of a detection overlap (view_iou: their mean pairwise IoU,
view_min_iou: the smallest) and writes their weighted mean around the view that agrees best with the others (include/t3d.h).  A box
that moves when the points are redrawn or mirrored is not a label: --min_view_iou A rejects a detection whose view_iou lies below A, where
the --min_* thresholds of consistency.py reject.  The reference has no such step: nothing runs it unless it is asked for.
"""
import ctypes as C

import numpy as np
import torch

from . import abi
from .abi import fptr, iptr
from .consistency import Test, lies_below

MAX_VIEWS = abi.DETECT_ENSEMBLE_MAX_VIEWS
FLAGS = ('tta', 'tta_flip', 'tta_vote_iou', 'min_view_iou')
TEST = Test('min_view_iou', ('view_iou',), 'view_iou < %g', lies_below, ())       # the stage's rejecting test (consistency.Test)


def check_options(tta=None, tta_flip=False, tta_vote_iou=None, min_view_iou=None):
    """The four options of the drivers -> (K or None, flip, vote threshold, min_view_iou or None); ValueError for K outside 2..8, a
    threshold outside [0, 1], or any of the other three given without K.  The vote threshold defaults to 0: every view that overlaps the
    anchor votes."""
    if tta is None:
        if tta_flip or tta_vote_iou is not None or min_view_iou is not None:
            raise ValueError('--tta_flip / --tta_vote_iou / --min_view_iou describe the views of --tta: they need --tta')
        return None, False, None, None
    K = int(tta)
    if K != tta or not 2 <= K <= MAX_VIEWS:
        raise ValueError('--tta must be a number of views in 2..%d, got %r' % (MAX_VIEWS, tta))
    vote = 0.0 if tta_vote_iou is None else float(tta_vote_iou)
    if not 0.0 <= vote <= 1.0:                       # (a NaN fails too)
        raise ValueError('--tta_vote_iou must lie in [0, 1], got %r' % (tta_vote_iou,))
    if min_view_iou is not None:
        min_view_iou = float(min_view_iou)
        if not 0.0 <= min_view_iou <= 1.0:
            raise ValueError('--min_view_iou must lie in [0, 1], got %r' % (min_view_iou,))
    return K, bool(tta_flip), vote, min_view_iou


def add_arguments(parser):
    parser.add_argument('--tta', type=int, default=None,
                        help='run every frustum through the network K times (2..%d), each view on a point draw of its own, and report the fused box and how well the views agree' % MAX_VIEWS)
    parser.add_argument('--tta_flip', action='store_true', help='with --tta: the odd views are mirrored in the centre view of the frustum')
    parser.add_argument('--tta_vote_iou', type=float, default=None,
                        help='with --tta: a view votes only above this IoU with the anchor view (0..1; default 0)')
    parser.add_argument('--min_view_iou', type=float, default=None,
                        help='with --tta: reject a detection whose mean pairwise IoU over its views lies below this (0..1)')


def view_seed(seed, v):
    """The seed of view v's point draw: view 0 keeps the run's own."""
    if v == 0:
        return int(seed)
    return (int(seed) * 1000003 + 7919 * v + 0x2545F491) & 0x7fffffff


def views_of(K, flip=False, seed=0):
    """[(seed, mirrored)] of the K views: view 0 is the seed and the orientation of the run without --tta; with `flip` the odd views
    are mirrored."""
    return [(view_seed(seed, v), bool(flip) and v % 2 == 1) for v in range(int(K))]


def flip_mask_of(views):
    return sum(1 << v for v, (_, flipped) in enumerate(views) if flipped)


class EnsembleRequest:
    """What `semisup_infer.inference(decode='device', views=...)` needs: the views (`views_of`), the metric of their IoUs ('3d' / 'bev'),
    the IoU with the anchor above which a view votes, and the view_iou below which a detection is rejected (or None)."""

    def __init__(self, views, metric='3d', vote_threshold=0.0, min_view_iou=None):
        self.views = [(int(s), bool(f)) for s, f in views]
        if not 1 <= len(self.views) <= MAX_VIEWS:
            raise ValueError('%d views: an ensemble takes 1 to %d' % (len(self.views), MAX_VIEWS))
        if self.views[0][1]:
            raise ValueError('view 0 is the run as it is: it cannot be mirrored')
        if metric not in abi.NMS_METRICS:
            raise ValueError("the metric is one of %s, got %r" % (tuple(abi.NMS_METRICS), metric))
        self.metric, self.vote_threshold, self.min_view_iou = metric, float(vote_threshold), min_view_iou

    def __len__(self):
        return len(self.views)

    @property
    def flip_mask(self):
        return flip_mask_of(self.views)


def log_line(req, d):
    """One line on a run's views: how many, how many mirrored, how many boxes were fused, the mean view_iou."""
    n = len(d.view_iou)
    return 'tta: %d views (%d mirrored), fused %d of %d boxes, mean view IoU %.4f' % (
        len(req), sum(f for _, f in req.views), int((d.n_views_voted > 0).sum()), n, float(d.view_iou.mean()) if n else 0.0)


class DeviceEnsemble:
    """Workspace and outputs of t3d_detect_ensemble: `run` launches on device tensors and owns label_out [n, 7], corners_out [n, 24],
    agreement [n], min_iou [n], anchor [n] and n_votes [n] until its next run."""

    def __init__(self, rt):
        self.rt = rt
        self.workspace = self.label = self.corners = self.agreement = self.min_iou = self.anchor = self.n_votes = None
        self._held = ()

    def run(self, labels, weights, corners0, flip_mask=0, rot_angle=None, vote_threshold=0.0, metric='3d', fill=None):
        """labels: per view [n, 7], weights: per view [n], corners0 [n, 8, 3] / [n, 24], rot_angle [n] or None: fp32 on the runtime's
        device, none of them written.  -> (label_out, corners_out, agreement, min_iou, anchor, n_votes).  fill: six values the outputs
        hold before the launch (default: whatever they held)."""
        rt = self.rt
        V, n = len(labels), int(weights[0].numel())
        assert len(weights) == V and corners0.numel() == n * 24
        assert all(t.numel() == n * 7 for t in labels) and all(t.numel() == n for t in weights) and (rot_angle is None or rot_angle.numel() >= n)
        held = list(labels) + list(weights) + [corners0] + ([] if rot_angle is None else [rot_angle])
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in held)
        if V > MAX_VIEWS:
            raise abi.T3DError('t3d_detect_ensemble: T3D_ERR_SHAPE (%d views, at most %d)' % (V, MAX_VIEWS))
        self.label, self.corners = abi.grown(self.label, n, torch.float32, rt.device, 7), abi.grown(self.corners, n, torch.float32, rt.device, 24)
        self.agreement, self.min_iou = (abi.grown(t, n, torch.float32, rt.device) for t in (self.agreement, self.min_iou))
        self.anchor, self.n_votes = (abi.grown(t, n, torch.int32, rt.device) for t in (self.anchor, self.n_votes))
        out = (self.label[:n], self.corners[:n], self.agreement[:n], self.min_iou[:n], self.anchor[:n], self.n_votes[:n])
        if fill is not None:
            for t, v in zip(out, fill):
                t.fill_(v)
        self.workspace = abi.grown(self.workspace, (abi.detect_ensemble_workspace_bytes(n, V) + 7) // 8, torch.int64, rt.device)
        self._held = held                                     # alive until the launches have run
        a = abi.DetectEnsembleArgs(n=n, V=V, metric=abi.NMS_METRICS[metric], flip_mask=int(flip_mask), vote_threshold=float(vote_threshold),
                                   rot_angle=fptr(rot_angle), corners0=fptr(corners0), workspace=C.c_void_p(self.workspace.data_ptr()),
                                   workspace_bytes=self.workspace.numel() * 8, label_out=fptr(out[0]), corners_out=fptr(out[1]),
                                   agreement=fptr(out[2]), min_iou=fptr(out[3]), anchor=iptr(out[4]), n_votes=iptr(out[5]))
        for v in range(V):
            a.label[v], a.weight[v] = fptr(labels[v]), fptr(weights[v])
        self._args = a
        self.relaunch()
        return out

    def relaunch(self):
        """The launches of the last `run` again, on the same buffers (tools/bench_detect_ensemble.py times them)."""
        abi.check(self.rt.lib.t3d_detect_ensemble(C.byref(self._args), self.rt.stream()), 't3d_detect_ensemble')
