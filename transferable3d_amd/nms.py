"""Per-image, per-class greedy 3-D non-maximum suppression on the device (t3d_detect_nms, csrc/nms.hip).

A 2-D detector hands over several overlapping boxes of one object; each becomes a frustum and a 3-D box of the same thing, and
script_3Deval.m credits only the first of them.  `DeviceNms.run` suppresses, inside every (image, class) group, any box that overlaps a
better-ranked kept box by more than a threshold -- on the corners t3d_detect_decode wrote, which never visit the host in between.
The reference has no such step: nothing runs it unless it is asked for (detect --nms_iou, semisup_infer --device_decode --nms_iou).

`DeviceFuse.run` (t3d_detect_fuse, csrc/fuse.hip; --nms_fuse) follows it on the same buffers: who is kept stays, and every kept box takes
the weighted mean geometry of the boxes it suppressed -- several estimates of one object, which the suppression alone throws away.

`DeviceNmsSweep.run` (t3d_detect_nms_sweep, csrc/nms_sweep.hip; detect --sweep) is `DeviceNms.run` for many configurations at once -- a
threshold out of up to 16 and a subset of the boxes each -- with every pair's IoU computed once (sweep.py chooses thresholds with it).

`DeviceSoftNms.run` (t3d_detect_soft_nms, csrc/soft_nms.hip; --soft_nms) is the alternative to `DeviceNms.run` where true neighbours overlap
(chairs in a row): a box that overlaps a better one is not dropped, its confidence is multiplied down by a function of the IoU (Soft-NMS,
Bodla et al., ICCV 2017), so a duplicate sinks to the tail of the ranked list while a neighbour keeps most of its confidence.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import abi
from .abi import fptr, iptr

METRICS = tuple(abi.NMS_METRICS)          # '3d': volume IoU, 'bev': IoU of the ground-plane rectangles
SCORES = ('prob', 'score')                # rank by the 2-D detection confidence / by the decoded network score
SOFT_METHODS = ('gaussian', 'linear')     # Soft-NMS: score *= exp(-IoU^2 / sigma) for IoU > 0 / score *= 1 - IoU for IoU > threshold


def check_options(nms_iou, nms_metric=None, nms_score=None):
    """The three options of the drivers -> (threshold or None, metric name, score name); ValueError for a threshold outside (0, 1], an
    unknown name, or a metric / score given without a threshold."""
    if nms_iou is None:
        if nms_metric is not None or nms_score is not None:
            raise ValueError('--nms_metric / --nms_score need --nms_iou')
        return None, '3d', 'prob'
    t = float(nms_iou)
    if not 0.0 < t <= 1.0:
        raise ValueError('--nms_iou must lie in (0, 1], got %r' % (nms_iou,))
    metric, score = nms_metric or '3d', nms_score or 'prob'
    if metric not in METRICS:
        raise ValueError('--nms_metric is one of %s, got %r' % (METRICS, metric))
    if score not in SCORES:
        raise ValueError('--nms_score is one of %s, got %r' % (SCORES, score))
    return t, metric, score


def check_fuse_options(nms_iou, nms_fuse=False, nms_fuse_iou=None):
    """The two box-voting options of the drivers -> (fuse, vote threshold or None).  nms_fuse_iou implies nms_fuse and defaults to
    nms_iou; ValueError without nms_iou, and for a vote threshold outside [nms_iou, 1]: every member of a cluster overlaps its kept box
    by more than nms_iou, so a lower value would silently change nothing."""
    if not nms_fuse and nms_fuse_iou is None:
        return False, None
    if nms_iou is None:
        raise ValueError('--nms_fuse / --nms_fuse_iou fuse the clusters of --nms_iou: they need --nms_iou')
    t = float(nms_iou) if nms_fuse_iou is None else float(nms_fuse_iou)
    if not float(nms_iou) <= t <= 1.0:
        raise ValueError('--nms_fuse_iou must lie in [--nms_iou, 1] = [%r, 1], got %r' % (nms_iou, nms_fuse_iou))
    return True, t


SoftOptions = collections.namedtuple('SoftOptions', 'method threshold sigma min_prob metric')


def check_soft_options(soft_nms=None, soft_nms_sigma=None, soft_nms_min_prob=None, nms_iou=None, nms_metric=None, nms_score=None, nms_fuse=False,
                       nms_fuse_iou=None):
    """The Soft-NMS options of the drivers beside the ones they share with the hard suppression -> None without soft_nms, else
    SoftOptions(method, threshold or None, sigma, min_prob, metric name).  'gaussian' decays every overlapping box by exp(-IoU^2 /
    sigma) and takes no threshold; 'linear' decays a box above the IoU nms_iou by 1 - IoU and needs it.  ValueError for an unknown method,
    sigma not a finite number above 0, min_prob outside [0, 1), a threshold with 'gaussian' or none with 'linear', for what cannot go with
    a decay -- ranking by the decoded score (the decay acts on the confidence the evaluation ranks by) and box voting (there are no
    clusters) -- and for a soft_nms_* option without soft_nms."""
    if soft_nms is None:
        if soft_nms_sigma is not None or soft_nms_min_prob is not None:
            raise ValueError('--soft_nms_sigma / --soft_nms_min_prob need --soft_nms')
        return None
    if soft_nms not in SOFT_METHODS:
        raise ValueError('--soft_nms is one of %s, got %r' % (SOFT_METHODS, soft_nms))
    if nms_score not in (None, 'prob'):
        raise ValueError('--soft_nms decays the 2-D detection confidence, which the evaluation ranks by: it does not go with --nms_score %s' % nms_score)
    if nms_fuse or nms_fuse_iou is not None:
        raise ValueError('--soft_nms suppresses nothing into clusters: it does not go with --nms_fuse / --nms_fuse_iou')
    metric = nms_metric or '3d'
    if metric not in METRICS:
        raise ValueError('--nms_metric is one of %s, got %r' % (METRICS, metric))
    sigma = 0.5 if soft_nms_sigma is None else float(soft_nms_sigma)
    floor = 0.001 if soft_nms_min_prob is None else float(soft_nms_min_prob)
    if not (0.0 < sigma < float('inf')):
        raise ValueError('--soft_nms_sigma must be a finite number above 0, got %r' % (soft_nms_sigma,))
    if not 0.0 <= floor < 1.0:
        raise ValueError('--soft_nms_min_prob must lie in [0, 1), got %r' % (soft_nms_min_prob,))
    if soft_nms == 'gaussian':
        if nms_iou is not None:
            raise ValueError('--soft_nms gaussian decays every overlapping box and has no threshold: it does not go with --nms_iou')
        return SoftOptions('gaussian', None, sigma, floor, metric)
    if soft_nms_sigma is not None:
        raise ValueError('--soft_nms_sigma is the width of --soft_nms gaussian: it does not go with --soft_nms linear')
    if nms_iou is None:
        raise ValueError('--soft_nms linear decays the boxes above an IoU threshold: it needs --nms_iou')
    return SoftOptions('linear', check_options(nms_iou)[0], sigma, floor, metric)


class Suppression(collections.namedtuple('Suppression', 'nms_iou nms_metric nms_score nms_fuse nms_fuse_iou soft')):
    """The suppression options of the drivers, checked and with their defaults (`suppression`): the threshold of the hard suppression or
    None, the metric name, the score name, whether the kept boxes are fused, the IoU above which a suppressed box votes (or None), and
    `soft`, the SoftOptions of Soft-NMS or None.  With `soft` the hard suppression stays off -- nms_iou None, no fusion, ranked by
    'prob' -- the threshold of 'linear' travels in `soft`, and nms_metric is its metric (the views of --tta read it there)."""
    __slots__ = ()

    @property
    def on(self):
        """Whether a suppression, hard or soft, was asked for."""
        return self.nms_iou is not None or self.soft is not None


def suppression(soft_nms=None, soft_nms_sigma=None, soft_nms_min_prob=None, nms_iou=None, nms_metric=None, nms_score=None, nms_fuse=False,
                nms_fuse_iou=None):
    """The eight suppression options of the drivers -> Suppression; ValueError as check_soft_options, check_options and
    check_fuse_options raise it, in that order."""
    soft = check_soft_options(soft_nms, soft_nms_sigma, soft_nms_min_prob, nms_iou, nms_metric, nms_score, nms_fuse, nms_fuse_iou)
    if soft is not None:
        return Suppression(None, soft.metric, 'prob', False, None, soft)
    t, metric, score = check_options(nms_iou, nms_metric, nms_score)
    return Suppression(t, metric, score, *check_fuse_options(t, nms_fuse, nms_fuse_iou), None)


def add_arguments(parser):
    parser.add_argument('--soft_nms', choices=SOFT_METHODS, default=None,
                        help="Soft-NMS: per image and class, a box that overlaps a better one keeps its place and its confidence is multiplied down -- 'gaussian': by exp(-IoU^2 / sigma); 'linear': by 1 - IoU above --nms_iou (which it needs); decayed confidences below --soft_nms_min_prob are dropped")
    parser.add_argument('--soft_nms_sigma', type=float, default=None, help='--soft_nms gaussian: the width sigma (> 0; default 0.5)')
    parser.add_argument('--soft_nms_min_prob', type=float, default=None,
                        help='--soft_nms: a detection whose decayed confidence falls below this is dropped (in [0, 1); default 0.001)')
    parser.add_argument('--nms_iou', type=float, default=None,
                        help='suppress, per image and class, a 3-D box that overlaps a better-ranked kept box by more than this IoU (0 < T <= 1; default: no suppression)')
    parser.add_argument('--nms_metric', choices=METRICS, default=None, help="IoU of --nms_iou: '3d' (volume, default) or 'bev' (ground plane)")
    parser.add_argument('--nms_score', choices=SCORES, default=None,
                        help="rank by the 2-D detection confidence ('prob', default: the last column of the result files) or by the decoded network score")
    parser.add_argument('--nms_fuse', action='store_true',
                        help='with --nms_iou: every kept box takes the weighted mean geometry of the boxes it suppressed (box voting); which boxes are kept, and every score, stay')
    parser.add_argument('--nms_fuse_iou', type=float, default=None,
                        help='a suppressed box votes only above this IoU with its kept box (in [--nms_iou, 1]; default --nms_iou: every suppressed box votes); implies --nms_fuse')


def groups_of(image_ids, class_ids):
    """(group_offsets [n_groups + 1], members [n]) int32: one group per distinct (image, class) pair, groups in ascending (image, class)
    order, box indices ascending inside a group."""
    img, cls = np.asarray(image_ids, np.int64).reshape(-1), np.asarray(class_ids, np.int64).reshape(-1)
    if img.shape != cls.shape:
        raise ValueError('%d image ids, %d class ids' % (len(img), len(cls)))
    n = len(img)
    if n == 0:
        return np.zeros(1, np.int32), np.zeros(0, np.int32)
    members = np.lexsort((np.arange(n), cls, img))
    si, sc = img[members], cls[members]
    starts = np.nonzero(np.concatenate([[True], (si[1:] != si[:-1]) | (sc[1:] != sc[:-1])]))[0]
    return np.concatenate([starts, [n]]).astype(np.int32), members.astype(np.int32)


def _lists(rt, group_offsets, members, n):
    """The lists of groups_of over n boxes, checked and uploaded -> (n_groups, max_group, and the two lists as int32 device
    tensors; an empty member list as one zero)."""
    go, mem = np.ascontiguousarray(group_offsets, np.int32), np.ascontiguousarray(members, np.int32)
    n_groups = len(go) - 1
    max_group = int(np.diff(go).max()) if n_groups > 0 else 0
    if n_groups < 0 or go[0] != 0 or (n_groups > 0 and (np.diff(go).min() < 0 or go[-1] != len(mem))) or len(mem) > n:
        raise ValueError('group_offsets / members are not the lists of groups_of')
    if len(mem) and (mem.min() < 0 or mem.max() >= n):
        raise ValueError('a member is not a box index of [0, %d)' % n)
    d_go, d_mem = torch.from_numpy(go).to(rt.device), torch.from_numpy(mem if len(mem) else np.zeros(1, np.int32)).to(rt.device)
    return n_groups, max_group, d_go, d_mem


def _boxes_and_lists(rt, corners, score, group_offsets, members):
    """What the three suppressions take alike: corners [n, 8, 3] / [n, 24] and score [n], fp32 and contiguous on the runtime's device,
    and the lists of groups_of -> (n, and what _lists answers)."""
    n = int(score.numel())
    assert corners.numel() == n * 24 and corners.is_contiguous() and score.is_contiguous()
    assert corners.dtype == torch.float32 and score.dtype == torch.float32
    return (n,) + _lists(rt, group_offsets, members, n)


class DeviceNms:
    """Workspace and outputs of t3d_detect_nms; `run` launches on device tensors.  The buffers grow as needed and are reused (abi.grown)."""

    def __init__(self, rt):
        self.rt = rt
        self.workspace = self.keep = self.suppressed_by = self.rank = None
        self._held = ()

    def run(self, corners, score, group_offsets, members, threshold, metric='3d', fill=None):
        """corners [n, 8, 3] / [n, 24] fp32 and score [n] fp32 on the runtime's device; group_offsets, members: NumPy / lists (uploaded:
        integers only) -> (keep uint8 [n], suppressed_by int32 [n], rank int32 [n]) device tensors, owned by this object until the
        next run.  fill: (keep, suppressed_by, rank) values the outputs hold before the launch (what a box in no group keeps; default
        1, -1, -1: an unlisted box is a kept one)."""
        rt = self.rt
        n, n_groups, max_group, d_go, d_mem = _boxes_and_lists(rt, corners, score, group_offsets, members)
        fk, fs, fr = (1, -1, -1) if fill is None else fill
        self.keep = abi.grown(self.keep, n, torch.uint8, rt.device)
        self.suppressed_by, self.rank = (abi.grown(t, n, torch.int32, rt.device) for t in (self.suppressed_by, self.rank))
        keep, sup, rank = self.keep[:n], self.suppressed_by[:n], self.rank[:n]
        keep.fill_(fk)
        sup.fill_(fs)
        rank.fill_(fr)
        need = abi.detect_nms_workspace_bytes(n, max_group)
        self.workspace = abi.grown(self.workspace, (need + 7) // 8, torch.int64, rt.device)
        self._held = (corners, score, d_go, d_mem)            # alive until the launches have run
        a = abi.DetectNmsArgs(n, n_groups, abi.NMS_METRICS[metric], fptr(corners), fptr(score), iptr(d_go), iptr(d_mem), float(threshold),
                              max_group, C.c_void_p(self.workspace.data_ptr()), self.workspace.numel() * 8, abi.u8ptr(keep), iptr(sup), iptr(rank))
        self._args = a
        self.relaunch()
        return keep, sup, rank

    def relaunch(self):
        """The launches of the last `run` again, on the same buffers (tools/bench_detect_nms.py times them alone)."""
        abi.check(self.rt.lib.t3d_detect_nms(C.byref(self._args), self.rt.stream()), 't3d_detect_nms')


class DeviceSoftNms:
    """Outputs of t3d_detect_soft_nms; `run` launches on device tensors.  The buffers grow as needed and are reused."""

    def __init__(self, rt):
        self.rt = rt
        self.score_out = self.keep = self.suppressed_by = self.n_decays = None
        self._held = ()

    def run(self, corners, score, group_offsets, members, method, threshold=None, sigma=0.5, min_score=0.001, metric='3d', fill=None):
        """corners [n, 8, 3] / [n, 24] fp32 and score [n] fp32 on the runtime's device; group_offsets, members: NumPy / lists, as for
        DeviceNms.run; method 'gaussian' (sigma) or 'linear' (threshold); min_score: the floor below which a decayed box is pruned.
        -> (score_out fp32 [n], keep uint8 [n], suppressed_by int32 [n], n_decays int32 [n]) device tensors, owned by this object until
        the next run.  fill: (score_out, keep, suppressed_by, n_decays) values the outputs hold before the launch (what a box in no
        group keeps; default: its input score, 1, -1, 0: an unlisted box is a kept one that nothing decayed)."""
        rt = self.rt
        if method not in SOFT_METHODS:
            raise ValueError('method is one of %s, got %r' % (SOFT_METHODS, method))
        if method == 'linear' and threshold is None:
            raise ValueError("method 'linear' needs a threshold")
        n, n_groups, max_group, d_go, d_mem = _boxes_and_lists(rt, corners, score, group_offsets, members)
        self.score_out, self.keep = abi.grown(self.score_out, n, torch.float32, rt.device), abi.grown(self.keep, n, torch.uint8, rt.device)
        self.suppressed_by, self.n_decays = (abi.grown(t, n, torch.int32, rt.device) for t in (self.suppressed_by, self.n_decays))
        out, keep, sup, dec = self.score_out[:n], self.keep[:n], self.suppressed_by[:n], self.n_decays[:n]
        if fill is None:
            out.copy_(score.view(-1))
        else:
            out.fill_(fill[0])
        fk, fs, fd = (1, -1, 0) if fill is None else fill[1:]
        keep.fill_(fk)
        sup.fill_(fs)
        dec.fill_(fd)
        self._held = (corners, score, d_go, d_mem)            # alive until the launch has run
        self._args = abi.DetectSoftNmsArgs(n, n_groups, abi.NMS_METRICS[metric], fptr(corners), fptr(score), iptr(d_go), iptr(d_mem),
                                           0.0 if threshold is None else float(threshold), max_group, abi.SOFT_NMS_METHODS[method], float(sigma),
                                           float(min_score), 0, None, 0, fptr(out), abi.u8ptr(keep), iptr(sup), iptr(dec))
        self.relaunch()
        return out, keep, sup, dec

    def relaunch(self):
        """The launch of the last `run` again, on the same buffers and on the working scores the last launch left: every listed box
        starts again from its input score (tools/bench_detect_soft_nms.py times it alone)."""
        abi.check(self.rt.lib.t3d_detect_soft_nms(C.byref(self._args), self.rt.stream()), 't3d_detect_soft_nms')


class DeviceFuse:
    """Workspace and outputs of t3d_detect_fuse behind a DeviceNms.run: `run` launches on device tensors and owns label_out [n, 7],
    corners_out [n, 24] and n_votes [n] until its next run."""

    def __init__(self, rt):
        self.rt = rt
        self.workspace = self.label = self.corners = self.n_votes = None
        self._held = ()

    def run(self, nms, label, corners, weight, vote_threshold, fill=None):
        """nms: the DeviceNms whose last `run` answered for these boxes (its keep / suppressed_by / rank and its lists are read where
        they lie); label [n, 7], corners [n, 8, 3] / [n, 24], weight [n]: fp32 on the runtime's device, none of them written.
        -> (label_out, corners_out, n_votes).  Before the launch the outputs hold copies of label and corners and n_votes 0 -- what a box
        in no group keeps; fill: (label value, corners value, n_votes value) to hold instead."""
        rt, a = self.rt, nms._args
        n = int(weight.numel())
        assert a.n == n and label.numel() == n * 7 and corners.numel() == n * 24
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (label, corners, weight))
        self.label, self.corners = abi.grown(self.label, n, torch.float32, rt.device, 7), abi.grown(self.corners, n, torch.float32, rt.device, 24)
        self.n_votes = abi.grown(self.n_votes, n, torch.int32, rt.device)
        lo, ko, nv = self.label[:n], self.corners[:n], self.n_votes[:n]
        if fill is None:
            lo.copy_(label.view(n, 7))
            ko.copy_(corners.view(n, 24))
            nv.zero_()
        else:
            lo.fill_(fill[0])
            ko.fill_(fill[1])
            nv.fill_(fill[2])
        self.workspace = abi.grown(self.workspace, (abi.detect_fuse_workspace_bytes(n) + 7) // 8, torch.int64, rt.device)
        self._held = (nms, label, corners, weight)            # alive until the launches have run
        self._args = abi.DetectFuseArgs(n, a.n_groups, a.metric, a.group_offsets, a.members, a.keep, a.suppressed_by, a.rank, fptr(label),
                                        fptr(corners), fptr(weight), float(vote_threshold), a.max_group,
                                        C.c_void_p(self.workspace.data_ptr()), self.workspace.numel() * 8, fptr(lo), fptr(ko), iptr(nv))
        self.relaunch()
        return lo, ko, nv

    def relaunch(self):
        """The launches of the last `run` again, on the same buffers (tools/bench_detect_fuse.py times them)."""
        abi.check(self.rt.lib.t3d_detect_fuse(C.byref(self._args), self.rt.stream()), 't3d_detect_fuse')


class DeviceNmsSweep:
    """Workspace and outputs of t3d_detect_nms_sweep (csrc/nms_sweep.hip): t3d_detect_nms for M configurations in one call, every pair's
    IoU computed once.  `run` launches on device tensors and owns keep [M, stride] and n_kept [M] until its next run."""

    def __init__(self, rt):
        self.rt = rt
        self.workspace = self.keep = self.n_kept = None
        self._held = ()

    def run(self, corners, score, group_offsets, members, thresholds, config_threshold, listed=None, metric='3d'):
        """corners [n, 8, 3] / [n, 24] fp32 and score [n] fp32 on the runtime's device; group_offsets, members: NumPy / lists, as for
        DeviceNms.run; thresholds: the 1 .. 16 distinct IoU thresholds of the grid; config_threshold [M]: per configuration the index
        of its threshold, or -1 for no suppression (NumPy / list: uploaded; or an int32 device tensor); listed: None (every box, in every
        configuration) or a uint8 device tensor [M, >= n] whose row m says which boxes take part in configuration m.
        -> (keep uint8 [M, n] -- a view of rows `stride` bytes apart, row m what DeviceNms.run answers for configuration m with the
        unlisted boxes left out of the groups and 0 for a box that is in no group or not listed -- and n_kept int32 [M])."""
        rt = self.rt
        n, n_groups, max_group, d_go, d_mem = _boxes_and_lists(rt, corners, score, group_offsets, members)
        thresholds = [float(t) for t in thresholds]
        K = len(thresholds)
        if not 1 <= K <= abi.NMS_SWEEP_MAX_THRESHOLDS:
            raise ValueError('%d NMS thresholds: one call takes 1 to %d' % (K, abi.NMS_SWEEP_MAX_THRESHOLDS))
        if torch.is_tensor(config_threshold):
            d_ct = config_threshold
            assert d_ct.dtype == torch.int32 and d_ct.is_contiguous()
        else:
            d_ct = torch.from_numpy(np.ascontiguousarray(config_threshold, np.int32).reshape(-1)).to(rt.device)
        M = int(d_ct.numel())
        if not 1 <= M <= abi.SWEEP_MAX_CONFIGS:
            raise ValueError('%d configurations: one call takes 1 to %d' % (M, abi.SWEEP_MAX_CONFIGS))
        listed_stride = 0
        if listed is not None:
            assert listed.dtype == torch.uint8 and listed.dim() == 2 and listed.shape[0] == M and listed.shape[1] >= n and listed.stride(1) == 1
            listed_stride = int(listed.stride(0)) if M > 1 else int(listed.shape[1])
        stride = max((n + 7) // 8 * 8, 8)                    # rows that start on 8 bytes are zeroed eight bytes at a time
        self.keep, self.n_kept = abi.grown(self.keep, M * stride, torch.uint8, rt.device), abi.grown(self.n_kept, M, torch.int32, rt.device)
        need = abi.detect_nms_sweep_workspace_bytes(n, max_group, K)
        self.workspace = abi.grown(self.workspace, (need + 7) // 8, torch.int64, rt.device)
        self._held = (corners, score, d_go, d_mem, d_ct, listed)            # alive until the launches have run
        a = abi.DetectNmsSweepArgs(n, n_groups, abi.NMS_METRICS[metric], fptr(corners), fptr(score), iptr(d_go), iptr(d_mem), max_group, K)
        for k, t in enumerate(thresholds):
            a.thresholds[k] = t
        a.M, a.listed_stride, a.keep_stride = M, listed_stride, stride
        a.config_threshold, a.listed = iptr(d_ct), abi.u8ptr(listed)
        a.workspace, a.workspace_bytes = C.c_void_p(self.workspace.data_ptr()), self.workspace.numel() * 8
        a.keep, a.n_kept = abi.u8ptr(self.keep), iptr(self.n_kept)
        self._args = a
        self.relaunch()
        return self.keep[:M * stride].view(M, stride)[:, :n], self.n_kept[:M]

    def relaunch(self):
        """The launches of the last `run` again, on the same buffers (tools/bench_detect_sweep.py times them alone)."""
        abi.check(self.rt.lib.t3d_detect_nms_sweep(C.byref(self._args), self.rt.stream()), 't3d_detect_nms_sweep')
