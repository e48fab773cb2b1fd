"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_detect_decode (include/t3d.h, csrc/detect.hip): `decode` is
the arithmetic on arrays of any float type, DetectDecodeSpec the entry point behind the ctypes struct on host pointers, so that
semisup_infer.inference(decode='device') and transferable3d_amd/detect.py run end to end through Runtime(device='cpu', lib=FakeDetectLib()).

`wide=True`: every float pointer of the struct is read and written as fp64 (the caller allocated its buffers that way, tests/
detect_check.WideRuntime).  The ABI is fp32; the wide form exists so that a test can compare result FILES with the reference's, which
print fp64 values at %f: an fp32 store of a value near 2 moves it by up to 1.2e-7, enough to turn over the sixth decimal of a printed value."""
import ctypes as C

import numpy as np

from fake_t3d import AbiSizeError, FakeLib, _struct, arr
from transferable3d_amd import abi
from transferable3d_amd.constants import MEAN_DIMS_ARR, NUM_HEADING_BIN as NH, NUM_SIZE_CLUSTER as NS

BOX = 3 + 2 * NH + 4 * NS


def get_3d_box(l, w, h, ry, center):
    """roi_seg_box3d_dataset.py:86-101, written out (not eval_det.get_3d_box: the tests compare the two)."""
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1]) * l / 2
    sy = np.array([1, 1, 1, 1, -1, -1, -1, -1]) * h / 2
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1]) * w / 2
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([c * sx + s * sz + center[0], sy + center[1], -s * sx + c * sz + center[2]], 1)


def decode(logits, box_out, stage1_center, total_delta=None, fit_prob=None, rot_angle=None):
    """logits [B,N,2], box_out [B,>=67], stage1_center [B,3], total_delta [B,7] | None, fit_prob [B] | None, rot_angle [B] | None ->
    dict of fp64 / integer arrays named as the struct's outputs."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    logits, box, s1, td, fit, rot = f(logits), f(box_out), f(stage1_center), f(total_delta), f(fit_prob), f(rot_angle)
    B = logits.shape[0]
    td = np.zeros((B, 7)) if td is None else td
    rot = np.zeros(B) if rot is None else rot
    l0, l1 = logits[:, :, 0], logits[:, :, 1]
    seg = l1 > l0
    with np.errstate(over='ignore'):
        p1 = 1.0 / (1.0 + np.exp(l0 - l1))
    cnt = seg.sum(1)
    mean_prob = np.where(seg, p1, 0.0).sum(1) / (cnt + 1)
    hs, ss = box[:, 3:3 + NH], box[:, 3 + 2 * NH:3 + 2 * NH + NS]
    hcls, scls = np.argmax(hs, 1), np.argmax(ss, 1)
    top = lambda x: 1.0 / np.exp(x - x.max(1, keepdims=True)).sum(1)
    score = np.log(mean_prob + 0.01) + np.log(top(hs) + 0.01) + np.log(top(ss) + 0.01)
    if fit is not None:
        score = score + np.log(fit + 0.01)
    r = np.arange(B)
    center = box[:, 0:3] + s1 - td[:, 0:3]
    hres = box[:, 3 + NH:3 + 2 * NH][r, hcls] * (np.pi / NH) - td[:, 6]
    sres = box[:, 3 + 2 * NH + NS:BOX].reshape(B, NS, 3)[r, scls] * MEAN_DIMS_ARR[scls] - td[:, 3:6]
    lwh = MEAN_DIMS_ARR[scls] + sres
    ry = hcls * (2 * np.pi / NH) + hres
    ry = np.where(ry > np.pi, ry - 2 * np.pi, ry) + rot
    c, s = np.cos(-rot), np.sin(-rot)
    tx, tz = c * center[:, 0] - s * center[:, 2], s * center[:, 0] + c * center[:, 2]
    ty = center[:, 1] + lwh[:, 2] / 2.0
    label = np.stack([lwh[:, 2], lwh[:, 1], lwh[:, 0], tx, ty, tz, ry], 1)
    corners = np.stack([get_3d_box(lwh[b, 0], lwh[b, 1], lwh[b, 2], ry[b], (tx[b], ty[b] - lwh[b, 2] / 2.0, tz[b])) for b in range(B)])
    return dict(seg=seg.astype(np.uint8), score=score, mask_count=cnt.astype(np.int32), heading_cls=hcls.astype(np.int32),
                size_cls=scls.astype(np.int32), center=center, heading_res=hres, size_res=sres, label=label, corners=corners)


class DetectDecodeSpec:
    """Mix-in: t3d_detect_decode for a specification library (FakeLib and its subclasses)."""
    wide = False

    def t3d_detect_decode(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        B, N = p.B, p.N
        if B <= 0 or N <= 0 or p.n_valid < 0 or p.ld_box < BOX:
            return -2
        outs = ('score', 'mask_count', 'heading_cls', 'size_cls', 'center', 'heading_res', 'size_res', 'label', 'corners')
        if not p.logits or not p.box_out or not p.stage1_center or not all(getattr(p, k) for k in outs):
            return -1
        fl = (lambda ptr, *shape: arr(C.cast(ptr, abi.D), *shape)) if self.wide else arr
        n = min(B, p.n_valid)
        if n == 0:
            return 0
        opt = lambda ptr, *shape: fl(ptr, *shape)[:n] if ptr else None
        r = decode(fl(p.logits, B, N, 2)[:n], fl(p.box_out, B, p.ld_box)[:n], fl(p.stage1_center, B, 3)[:n], opt(p.total_delta, B, 7),
                   opt(p.fit_prob, B), opt(p.rot_angle, B))
        for k, shape in (('score', (B,)), ('center', (B, 3)), ('heading_res', (B,)), ('size_res', (B, 3)), ('label', (B, 7)),
                         ('corners', (B, 8, 3))):
            fl(getattr(p, k), *shape)[:n] = r[k]
        for k in ('mask_count', 'heading_cls', 'size_cls'):
            arr(getattr(p, k), B)[:n] = r[k]
        if p.seg:
            arr(p.seg, B, N)[:n] = r['seg']
        return 0


class FakeDetectLib(DetectDecodeSpec, FakeLib):
    def __init__(self, wide=False):
        FakeLib.__init__(self)
        self.wide = wide
