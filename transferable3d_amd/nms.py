"""Per-image, per-class greedy 3-D non-maximum suppression on the device (t3d_detect_nms, csrc/nms.hip).

A 2-D detector hands over several overlapping boxes of one object; each becomes a frustum and a 3-D box of the same thing, and
script_3Deval.m credits only the first of them.  `DeviceNms.run` suppresses, inside every (image, class) group, any box that overlaps a
better-ranked kept box by more than a threshold -- on the corners t3d_detect_decode wrote, which never visit the host in between.
The reference has no such step: nothing runs it unless it is asked for (detect --nms_iou, semisup_infer --device_decode --nms_iou).
"""
import ctypes as C

import numpy as np
import torch

from . import abi
from .abi import fptr, iptr

METRICS = tuple(abi.NMS_METRICS)          # '3d': volume IoU, 'bev': IoU of the ground-plane rectangles
SCORES = ('prob', 'score')                # rank by the 2-D detection confidence / by the decoded network score


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


def add_arguments(parser):
    parser.add_argument('--nms_iou', type=float, default=None,
                        help='suppress, per image and class, a 3-D box that overlaps a better-ranked kept box by more than this IoU (0 < T <= 1; default: no suppression)')
    parser.add_argument('--nms_metric', choices=METRICS, default=None, help="IoU of --nms_iou: '3d' (volume, default) or 'bev' (ground plane)")
    parser.add_argument('--nms_score', choices=SCORES, default=None,
                        help="rank by the 2-D detection confidence ('prob', default: the last column of the result files) or by the decoded network score")


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


class DeviceNms:
    """Workspace and outputs of t3d_detect_nms; `run` launches on device tensors.  The buffers grow as needed and are reused."""

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
        n = int(score.numel())
        assert corners.numel() == n * 24 and corners.is_contiguous() and score.is_contiguous()
        assert corners.dtype == torch.float32 and score.dtype == torch.float32
        go, mem = np.ascontiguousarray(group_offsets, np.int32), np.ascontiguousarray(members, np.int32)
        n_groups = len(go) - 1
        max_group = int(np.diff(go).max()) if n_groups > 0 else 0
        if n_groups < 0 or go[0] != 0 or (n_groups > 0 and (np.diff(go).min() < 0 or go[-1] != len(mem))) or len(mem) > n:
            raise ValueError('group_offsets / members are not the lists of groups_of')
        if len(mem) and (mem.min() < 0 or mem.max() >= n):
            raise ValueError('a member is not a box index of [0, %d)' % n)
        fk, fs, fr = (1, -1, -1) if fill is None else fill
        if self.keep is None or self.keep.numel() < n:
            new = lambda dtype: torch.zeros(max(n, 1), dtype=dtype, device=rt.device)      # (owned here, not by the runtime: they are replaced as they grow)
            self.keep, self.suppressed_by, self.rank = new(torch.uint8), new(torch.int32), new(torch.int32)
        keep, sup, rank = self.keep[:n], self.suppressed_by[:n], self.rank[:n]
        keep.fill_(fk)
        sup.fill_(fs)
        rank.fill_(fr)
        need = abi.detect_nms_workspace_bytes(n, max_group)
        if self.workspace is None or self.workspace.numel() * 8 < need:
            self.workspace = torch.zeros(max(need // 8, 1), dtype=torch.int64, device=rt.device)
        d_go, d_mem = torch.from_numpy(go).to(rt.device), torch.from_numpy(mem if len(mem) else np.zeros(1, np.int32)).to(rt.device)
        self._held = (corners, score, d_go, d_mem)            # alive until the launches have run
        a = abi.DetectNmsArgs(n, n_groups, abi.NMS_METRICS[metric], fptr(corners), fptr(score), iptr(d_go), iptr(d_mem), float(threshold),
                              max_group, C.c_void_p(self.workspace.data_ptr()), self.workspace.numel() * 8, abi.u8ptr(keep), iptr(sup), iptr(rank))
        self._args = a
        self.relaunch()
        return keep, sup, rank

    def relaunch(self):
        """The launches of the last `run` again, on the same buffers (tools/bench_detect_nms.py times them alone)."""
        abi.check(self.rt.lib.t3d_detect_nms(C.byref(self._args), self.rt.stream()), 't3d_detect_nms')
