"""Shared cases of the head / loss / optimiser kernel tests (tests/test_kernels_heads_gpu.py on libt3d.so, tests/test_kernels_heads_cpu.py on
fake_t3d.FakeLib): the launch forms of csrc/heads.hip, the stage-c glue of csrc/boxpc.hip, csrc/bn_optim.hip and the shapes of
t3d_weak_loss that the one-shape tests of tests/test_kernels_gpu.py do not reach.

A check here takes an `Env` (a library and the device its pointers live on), builds its inputs from a fixed seed, runs the fp64
specification (tests/fake_t3d.py) on host copies of the same inputs and the library ONCE on buffers of its own, and compares.  Every
tensor a launch writes comes from `Bufs.out` (tests/rider_check.py): filled with a NaN bit pattern and fenced by guard bands of 4096
words of the same pattern (more than a row of the widest tensor used here), so a store beside an output is seen, an element that was
not written shows as NaN, and rows / columns the kernel must leave alone are compared for their bits.  The tolerances are those of the
test of the same kernel in tests/test_kernels_gpu.py -- named where they are used -- or derived where they are used; none is measured.
Every comparison prints its worst error next to the bound that applied there (`_within` of tests/test_kernels_glue_gpu.py)."""
import ctypes as C
import functools

import numpy as np
import torch

import rider_check as rc
from fake_t3d import FakeLib, MEAN32, hash_keep_mask, strong_loss_f64
from rider_check import Bufs, Env, SENT, ERR_ARG, ERR_SHAPE
from test_kernels_glue_gpu import _close, _fit_logits, _same_bits, _within
from transferable3d_amd import abi
from transferable3d_amd.abi import fptr, iptr

SPEC = Env(FakeLib(), 'cpu')
NH, NS = 12, 10
F32 = np.float32


def call(env, name, a):
    return getattr(env.lib, name)(C.byref(a), env.stream())


def launch(env, name, build):
    """build(bufs) -> argument struct.  One launch on fresh buffers: (return code, snapshot of every written tensor)."""
    b = Bufs(env.dev)
    a = build(b)
    code = call(env, name, a)
    env.sync()
    return code, b.snapshot()


def both(env, name, build, what):
    """The specification and `env`'s library on the same case: (got, ref) snapshots; the guards of `got` are checked."""
    code, ref = launch(SPEC, name, build)
    assert code == 0, (what, 'spec', code)
    code, got = launch(env, name, build)
    assert code == 0, (what, code)
    rc.check_guards(got, what)
    return got, ref


def val(snap, name, shape, dtype=np.float32):
    n = int(np.prod(shape))
    return rc.body(snap, name, dtype)[:n].reshape(shape)


def words(snap, name):
    return rc.body(snap, name, np.int32)


def nan_cols(a, width):
    """`a` widened to `width` columns, the pad columns NaN (a kernel that reads them poisons its outputs)."""
    out = np.full((a.shape[0], width), np.nan, a.dtype)
    out[:, :a.shape[1]] = a
    return out


# ======================================================================================================================================
# 1. t3d_strong_loss / t3d_box_head_iou
# ======================================================================================================================================
STRONG_B = [1, 128, 129, 512, 513, 1024]        # both sides of the LDS / private switch (128) and of the summary-thread switch (512); the limit
HEAD_IOU_B = [1, 63, 64, 65, 200]               # k_box_head_iou runs 64-thread blocks
STRONG_W = (1.0, 1.0, 20.0, 1.0, 20.0, 1.0, 1.0, 0.1, 1.0)      # test_strong_loss's weights (= oracle default_config())
# planted rows (batches of 64 and more): one per arithmetic branch of k_strong_loss
ROW = dict(zero_center=5, zero_s1=6, zero_size=7, far=8, big_eh=9, flip=10, ties=11, clamp=12)
ZERO_ROWS = (ROW['zero_center'], ROW['zero_s1'], ROW['zero_size'])


def strong_inputs(B, all2d=False):
    """(a copy of the cached case: no caller can change it for the next)"""
    return {k: v.copy() for k, v in _strong_inputs(B, all2d).items()}


@functools.lru_cache(maxsize=None)
def _strong_inputs(B, all2d):
    r = np.random.RandomState(1000 + B)
    box = (r.normal(size=(B, 67)) * 0.4).astype(F32)
    s1 = (r.normal(size=(B, 3)) * 0.5).astype(F32)
    yc = (s1 + r.normal(size=(B, 3)) * 0.8).astype(F32)          # distances on both sides of the Huber deltas 1 and 2
    yoc, ydc = r.randint(0, NH, size=B).astype(np.int32), r.randint(0, NS, size=B).astype(np.int32)
    yor = r.uniform(-0.26, 0.26, size=B).astype(F32)
    ydr = (r.normal(size=(B, 3)) * 0.1).astype(F32)
    seg = np.abs(r.normal(size=B)).astype(F32)
    is2d = (r.uniform(size=B) < 0.3).astype(np.int32)
    for b in range(0, B, 2):                                     # half of the predicted bins agree with the label's: IoUs that are not all tiny
        box[b, 3 + yoc[b]] = 5.0
        box[b, 27 + ydc[b]] = 5.0
    for b in range(0, B, 4):
        yc[b] = (box[b, :3] + s1[b] + r.normal(size=3) * 0.1).astype(F32)
    if B >= 64:
        R = ROW
        is2d[list(R.values())] = 0
        # y_center == box[0:3] + stage1 exactly (eighths: the fp32 and the fp64 sum are the same number) and y_center == stage1 exactly
        box[R['zero_center'], 0:3], s1[R['zero_center']] = (0.25, -0.5, 0.125), (1.5, 0.75, -2.0)
        yc[R['zero_center']] = box[R['zero_center'], 0:3] + s1[R['zero_center']]
        yc[R['zero_s1']] = s1[R['zero_s1']]
        # size-residual error exactly 0: label residual = mean / 2 (a halving is exact, so is the quotient 0.5), prediction 0.5
        k = ydc[R['zero_size']]
        ydr[R['zero_size']] = MEAN32[k] * F32(0.5)
        box[R['zero_size'], 37 + 3 * k:40 + 3 * k] = 0.5
        yc[R['far']] = s1[R['far']] + F32(3.0)                               # beyond both Huber deltas
        box[R['big_eh'], 15 + yoc[R['big_eh']]], yor[R['big_eh']] = 2.5, 0.0      # |eh| > 1
        # predicted heading = label heading + pi, same sizes (mean + 2 * 0.125 mean = mean + 0.25 mean), centres 0.05 apart: the flipped
        # corner set wins (d1 > d2)
        b, j, k = R['flip'], yoc[R['flip']], ydc[R['flip']]
        box[b, 15 + j], yor[b], ydr[b], box[b, 37 + 3 * k:40 + 3 * k] = 12.0, 0.0, MEAN32[k] * F32(0.25), 0.125
        yc[b] = (box[b, :3] + s1[b]).astype(F32) + F32(0.05)
        # exact ties in the scores: the first arg-max (bins 2 and 1) wins in reg_theta / reg_dims and in the IoU
        b = R['ties']
        box[b, 3:15], box[b, 27:37] = box[b, 3:15] * 0.1, box[b, 27:37] * 0.1
        box[b, 3 + 2] = box[b, 3 + 7] = 3.0
        box[b, 27 + 1] = box[b, 27 + 4] = 3.0
        b = R['clamp']                                                     # size residual below -1 in the arg-max class: reg_dims = 1e-5
        box[b, 27:37] *= 0.1
        box[b, 27 + 3], box[b, 37 + 9:37 + 12] = 5.0, -1.5
    if all2d:
        is2d[:] = 1
    d = dict(box=box, s1=s1, yc=yc, yoc=yoc, ydc=ydc, yor=yor, ydr=ydr, seg=seg, is2d=is2d)
    return d


@functools.lru_cache(maxsize=None)
def strong_ref(B, all2d, with_seg, norm3d):
    """The fp64 specification of the case (shared by every launch form of it, unrounded)."""
    d = strong_inputs(B, all2d)
    return strong_loss_f64(d['box'], d['s1'], d['yc'], d['yoc'], d['yor'], d['ydc'], d['ydr'], d['is2d'], d['seg'] if with_seg else None,
                           abi.StrongWeights(*STRONG_W), norm3d, with_iou=True)


STRONG_OUT = (('dbox', 67), ('dstage1', 3), ('terms', 8), ('total_losses', 1), ('loss', 0), ('center', 3), ('reg_dims', 3), ('reg_theta', 1))


def strong_build(d, B, ld_box, with_iou, with_seg, norm3d, iou_only=None):
    def build(b):
        a = abi.StrongLossArgs()
        a.box, a.ld_box, a.stage1_center = fptr(b.inp(nan_cols(d['box'], max(ld_box, 67)))), ld_box, fptr(b.inp(d['s1']))
        a.seg_loss = fptr(b.inp(d['seg']) if with_seg else None)
        a.y_center, a.y_orient_cls, a.y_orient_reg = fptr(b.inp(d['yc'])), iptr(b.inp(d['yoc'])), fptr(b.inp(d['yor']))
        a.y_dims_cls, a.y_dims_reg, a.is_data_2D = iptr(b.inp(d['ydc'])), fptr(b.inp(d['ydr'])), iptr(b.inp(d['is2d']))
        a.wts, a.normalize_by_3d_count, a.B = abi.StrongWeights(*STRONG_W), norm3d, B
        a.dbox, a.dstage1, a.terms = fptr(b.out('dbox', (B, 67))), fptr(b.out('dstage1', (B, 3))), fptr(b.out('terms', (B, 8)))
        a.total_losses, a.loss, a.center = fptr(b.out('total_losses', B)), fptr(b.out('loss', 1)), fptr(b.out('center', (B, 3)))
        a.reg_dims, a.reg_theta = fptr(b.out('reg_dims', (B, 3))), fptr(b.out('reg_theta', B))
        if with_iou or iou_only == 'iou3d':
            a.iou3d = fptr(b.out('iou3d', B, init=np.zeros(B, F32) if iou_only else None))
        if with_iou or iou_only == 'iou2d':
            a.iou2d = fptr(b.out('iou2d', B, init=np.zeros(B, F32) if iou_only else None))
        a._keep = b
        return a
    return build


def head_iou_build(d, B, ld_box, with_s1=True):
    def build(b):
        a = abi.BoxHeadIouArgs(fptr(b.inp(nan_cols(d['box'], max(ld_box, 67)))), ld_box, fptr(b.inp(d['s1']) if with_s1 else None),
                               fptr(b.inp(d['yc'])), iptr(b.inp(d['yoc'])), fptr(b.inp(d['yor'])), iptr(b.inp(d['ydc'])), fptr(b.inp(d['ydr'])),
                               fptr(b.out('iou2d', B)), fptr(b.out('iou3d', B)), B)
        a._keep = b
        return a
    return build


def with_B(build, B):
    """The arguments of `build` with another batch size (the buffers stay those of the batch it was built for)."""
    def rebuilt(b):
        a = build(b)
        a.B = B
        return a
    return rebuilt


def check_strong_loss(env, B, with_iou, with_seg, norm3d, ld_box, all2d=False):
    d = strong_inputs(B, all2d)
    ref = strong_ref(B, all2d, with_seg, norm3d)
    tag = 'strong_loss B=%d iou=%d seg=%d norm3d=%d ld=%d%s ' % (B, with_iou, with_seg, norm3d, ld_box, ' all-2D' if all2d else '')
    code, got = launch(env, 't3d_strong_loss', strong_build(d, B, ld_box, with_iou, with_seg, norm3d))
    assert code == 0, (tag, code)
    rc.check_guards(got, tag)
    for k, w in STRONG_OUT:
        r = ref[k]
        # test_strong_loss's tolerance: rtol 1e-4, atol 2e-5 max|ref| of the output
        _close(tag + k, val(got, k, r.shape), r, 1e-4, 2e-5 * max(float(np.abs(r).max()), 1e-6))
    assert ('iou3d' in got) == with_iou
    if with_iou:
        # IoUs at 2e-5 absolute (test_box_head_iou_and_strong_loss_summary), and t3d_box_head_iou on the same inputs
        code, head = launch(env, 't3d_box_head_iou', head_iou_build(d, B, ld_box))
        assert code == 0
        rc.check_guards(head, tag + 'box_head_iou')
        for k in ('iou3d', 'iou2d'):
            _within(tag + k, val(got, k, B), ref[k], 2e-5)
            _within(tag + 'box_head_iou ' + k, val(head, k, B), ref[k], 2e-5)
            _within(tag + k + ' against box_head_iou', val(got, k, B), val(head, k, B).astype(np.float64), 2e-5)
        if not all2d:
            assert (ref['iou3d'] > 0.2).sum() >= max(1, B // 16), 'the case has no overlapping boxes'
    t = val(got, 'terms', (B, 8))
    if all2d:
        # w3d = 0 everywhere: with normalize_by_3d_count the sum is 0 / (0 + 1e-3)
        assert float(val(got, 'loss', 1)[0]) == 0.0 and not val(got, 'dbox', (B, 67)).any() and not val(got, 'dstage1', (B, 3)).any()
        assert not val(got, 'total_losses', B).any() and float(t[:, 1:].max()) > 0
    elif B >= 64:
        R = ROW
        assert t[R['zero_center'], 1] == 0 and t[R['zero_s1'], 2] == 0 and t[R['zero_size'], 6] == 0
        assert (val(got, 'reg_dims', (B, 3))[R['clamp']] == F32(1e-5)).all()
        g = val(got, 'dbox', (B, 67))
        assert g[R['zero_size'], 37:67].any(), 'the corner loss still reaches the size residuals of the zero-error row'
    return got


def strong_case_facts(B):
    """What the planted rows must be, from the inputs in fp64: (rows with an exactly zero distance, the flip row's d1 - d2 per corner)."""
    from oracle import ref_torch as R
    d = strong_inputs(B)
    box, s1, yc, ydr = [d[k].astype(np.float64) for k in ('box', 's1', 'yc', 'ydr')]
    mean = MEAN32.astype(np.float64)
    k = d['ydc']
    srn = box[:, 37:67].reshape(B, NS, 3)[np.arange(B), k]
    zero = (np.linalg.norm(yc - (box[:, :3] + s1), axis=1) == 0) | (np.linalg.norm(yc - s1, axis=1) == 0) | \
        (np.linalg.norm(srn - ydr / mean[k], axis=1) == 0)
    b = ROW['flip']
    t = lambda v: torch.as_tensor(np.atleast_2d(v))
    bins = np.arange(NH) * (2 * np.pi / NH)
    j = d['yoc'][b]
    th = bins[j] + box[b, 15 + j] * (np.pi / NH)
    cp = R.box3d_corners_helper(t(box[b, :3] + s1[b]), torch.as_tensor([th]), t(mean[k[b]] + 2 * srn[b] * mean[k[b]]))[0]
    hl = bins[j] + float(d['yor'][b])
    cg = R.box3d_corners_helper(t(yc[b]), torch.as_tensor([hl]), t(mean[k[b]] + ydr[b]))[0]
    cgf = R.box3d_corners_helper(t(yc[b]), torch.as_tensor([hl + np.pi]), t(mean[k[b]] + ydr[b]))[0]
    return np.nonzero(zero)[0], (torch.norm(cp - cg, dim=-1) - torch.norm(cp - cgf, dim=-1)).numpy()


def check_strong_spec_against_autograd(B, norm3d):
    """The spec's hand-derived backward against autograd of oracle/ref_torch.get_strong_loss in fp64, `ep` built from the 67 head
    columns by _slice_box_heads.  Rows with an exactly zero distance stay out (torch.norm has no gradient at 0; the kernel and the
    spec give that term none): asserted to be the three planted rows and no other.  The per-frustum terms and the gradients agree to
    1e-9 of each entry itself; an entry whose reference is zero must be zero."""
    from oracle import ref_torch as R
    d = strong_inputs(B)
    zero, _ = strong_case_facts(B)
    assert sorted(zero.tolist()) == sorted(ZERO_ROWS)
    rows = np.setdiff1d(np.arange(B), zero)
    assert len(rows) == B - len(ZERO_ROWS)
    ref = strong_ref(B, False, True, norm3d)
    f64 = lambda k: torch.as_tensor(d[k][rows].astype(np.float64))
    out, s1 = f64('box').requires_grad_(True), f64('s1').requires_grad_(True)
    ep = {'stage1_center': s1}
    R._slice_box_heads(out, s1, ep, '', torch.float64)
    n = len(rows)
    W = abi.StrongWeights(*STRONG_W)          # the weights as the struct holds them: fp32 (0.1 is not 0.1)
    c = R.default_config(STRONG_BOX_MULTIPLER=W.box_multiplier, STRONG_WEIGHT_CENTER=W.center, STRONG_WEIGHT_ORIENT_CLS=W.orient_cls,
                         STRONG_WEIGHT_ORIENT_REG=W.orient_reg, STRONG_WEIGHT_DIMS_CLS=W.dims_cls, STRONG_WEIGHT_DIMS_REG=W.dims_reg,
                         STRONG_WEIGHT_TNET_CENTER=W.tnet_center, STRONG_WEIGHT_CORNER=W.corner)
    labels = (torch.zeros(n, 1, dtype=torch.int64), f64('yc'), torch.as_tensor(d['yoc'][rows]), f64('yor'), torch.as_tensor(d['ydc'][rows]), f64('ydr'))
    _, box_l = R.get_strong_loss((torch.zeros(n, 1, 2, dtype=torch.float64), None), labels, ep, c)
    w3d = torch.as_tensor((1 - d['is2d']).astype(np.float64))
    norm = 1.0 / (float(w3d.sum()) + 1e-3) if norm3d else 1.0 / B
    g_out, g_s1 = torch.autograd.grad((w3d[rows] * box_l).sum() * norm, [out, s1])
    terms = ep['loss_terms']
    want_terms = torch.stack([terms[k] for k in ('center', 'stage1', 'hcls', 'hres', 'scls', 'sres', 'corner')], 1).detach().numpy()
    tag = 'strong spec vs autograd B=%d norm3d=%d ' % (B, norm3d)
    _within(tag + 'terms', ref['terms'][rows, 1:], want_terms, 1e-9 * np.abs(want_terms))
    _within(tag + 'dbox', ref['dbox'][rows], g_out.numpy(), 1e-9 * np.abs(g_out.numpy()))
    _within(tag + 'dstage1', ref['dstage1'][rows], g_s1.numpy(), 1e-9 * np.abs(g_s1.numpy()))
    assert float(g_out.abs().max()) > 0 and float(g_s1.abs().max()) > 0


def check_strong_refusals(env):
    d = strong_inputs(64)
    for B in (0, 1025):                                               # (buffers of a batch the launcher takes: only B is wrong)
        code, snap = launch(env, 't3d_strong_loss', with_B(strong_build(strong_inputs(1024), 1024, 67, True, True, 0), B))
        assert code == ERR_SHAPE, B
        assert all((words(snap, k) == SENT).all() for k in snap)
    for only in ('iou2d', 'iou3d'):                                   # exactly one of the two IoU outputs
        code, _ = launch(env, 't3d_strong_loss', strong_build(d, 64, 67, False, True, 0, iou_only=only))
        assert code == ERR_ARG, only
    code, snap = launch(env, 't3d_strong_loss', strong_build(d, 64, 66, True, True, 0))      # a row narrower than the 67 heads
    assert code == ERR_SHAPE
    for k in snap:
        assert (words(snap, k) == SENT).all(), k                      # a refused call writes nothing


def check_box_head_iou(env, B, ld_box, with_s1):
    d = strong_inputs(max(B, 64))
    d = {k: np.ascontiguousarray(v[:B]) for k, v in d.items()}
    tag = 'box_head_iou B=%d ld=%d s1=%d ' % (B, ld_box, with_s1)
    got, ref = both(env, 't3d_box_head_iou', head_iou_build(d, B, ld_box, with_s1), tag)
    for k in ('iou3d', 'iou2d'):
        _within(tag + k, val(got, k, B), val(ref, k, B), 2e-5)


def check_box_head_iou_refusals(env):
    d = strong_inputs(64)
    code, snap = launch(env, 't3d_box_head_iou', head_iou_build(d, 64, 66))
    assert code == ERR_SHAPE and (words(snap, 'iou3d') == SENT).all()
    code, snap = launch(env, 't3d_box_head_iou', with_B(head_iou_build(d, 64, 67), 0))
    assert code == ERR_SHAPE and (words(snap, 'iou3d') == SENT).all()


# ======================================================================================================================================
# 2. stage-c glue
# ======================================================================================================================================
NARROW_SHAPES = [(64, 128, 0, 1, 1), (192, 384, 4, 6, 8), (128, 256, 0, 8, 8), (64, 384, 3, 5, 7), (64, 128, 0, 4, 4)]      # M, N, k0, kn, ld_out


def _bf16_values(a):
    return torch.as_tensor(a).bfloat16().float().numpy()


def narrow_build(env, M, N, k0, kn, ld_out, bf16):
    r = np.random.RandomState(M + N + 10 * k0 + kn)
    dz, y = _bf16_values((r.normal(size=(M, N)) * 1e-2).astype(F32)), _bf16_values(r.normal(size=(M, N)).astype(F32))
    coef, w = r.normal(size=(3, N)).astype(F32), r.normal(size=(k0 + kn, N)).astype(F32)

    def build(b):
        as16 = bf16 and b.dev.type != 'cpu'                 # (the fp32 spec reads the same numbers: they are bf16-representable)
        t = [b.inp(v) for v in (dz, y)]
        if as16:
            t = [v.bfloat16() for v in t]
            b.keep.extend(t)
        a = abi.DgradNarrowArgs(abi.DySrc(fptr(t[0]), fptr(t[1]), fptr(b.inp(coef)), iptr(None), fptr(None), abi.BF16 if as16 else abi.F32),
                                fptr(b.inp(w)), k0, kn, fptr(b.out('out', (M, ld_out))), ld_out, M, N)
        a._keep = b
        return a
    return build


def check_dgrad_narrow(env, M, N, k0, kn, ld_out, bf16):
    tag = 'dgrad_narrow M=%d N=%d k0=%d kn=%d ld=%d %s ' % (M, N, k0, kn, ld_out, 'bf16' if bf16 else 'f32')
    got, ref = both(env, 't3d_pointmlp_dgrad_narrow', narrow_build(env, M, N, k0, kn, ld_out, bf16), tag)
    g, r = val(got, 'out', (M, ld_out)), val(ref, 'out', (M, ld_out))
    # test_stage_c_glue_kernels: rtol 1e-4, atol 1e-4 max|ref|
    _close(tag + 'out', g[:, :kn], r[:, :kn], 1e-4, 1e-4 * float(np.abs(r[:, :kn]).max()))
    assert (val(got, 'out', (M, ld_out), np.int32)[:, kn:] == SENT).all(), tag + 'the columns behind kn were written'


def check_dgrad_narrow_refusals(env):
    for M, N, k0, kn, ld_out in ((96, 128, 0, 4, 4), (64, 192, 0, 4, 4), (64, 128, 0, 0, 4), (64, 128, 0, 9, 12), (64, 128, 0, 6, 5)):
        b = Bufs(env.dev)
        z = b.inp(np.zeros((128, 256), F32))
        a = abi.DgradNarrowArgs(abi.DySrc(fptr(z), fptr(z), fptr(z), iptr(None), fptr(None), abi.F32), fptr(z), k0, kn,
                                fptr(b.out('out', (128, 16))), ld_out, M, N)
        assert call(env, 't3d_pointmlp_dgrad_narrow', a) == ERR_SHAPE, (M, N, k0, kn, ld_out)
        env.sync()
        assert (words(b.snapshot(), 'out') == SENT).all()


SEMI_B = [1, 7, 32, 1024]
TRAINED = (1, 2, 6, 7, 8)          # test_stage_c_glue_kernels's trained classes; class 8 gets no member, class 6 exactly one


def semi_inputs(B):
    r = np.random.RandomState(400 + B)
    members = np.array([0, 1, 2, 3, 4, 5, 7, 9])          # never 6 or 8
    cls = members[r.randint(0, len(members), size=B)]
    if B >= 7:
        cls[3], cls[4] = 6, 2                              # class 6: a single member (e = 0 exactly); class 2: row 4 and the soft row 5
    oh = np.eye(10, dtype=F32)[cls]
    if B >= 7:
        oh[5] = 0.05                                       # a soft vector with a tie: classes 2 and 7 at 0.3, the first wins
        oh[5, 2] = oh[5, 7] = 0.3
        cls[5] = 2
    out9 = r.normal(size=(B, 9)).astype(F32)
    out9[:, 7:9] = _fit_logits(r, B)
    return dict(strong=np.array([3.25], F32), dims=(1.0 + r.normal(size=(B, 3)) * 0.8).astype(F32), oh=oh, cls=cls,
                is2d=(r.uniform(size=B) < 0.5).astype(np.int32), out9=out9)


def check_semi_final_loss(env, B, only2d, variant):
    d = semi_inputs(B)
    trained = () if variant == 'T0' else TRAINED
    w_weak = 0.0 if variant == 'w_weak0' else 0.1

    def build(b):
        a = abi.SemiFinalLossArgs()
        a.strong_loss, a.reg_dims, a.one_hot = fptr(b.inp(d['strong'])), fptr(b.inp(d['dims'])), fptr(b.inp(d['oh']))
        a.is_data_2D, a.out9 = iptr(b.inp(d['is2d'])), fptr(b.inp(d['out9']))
        for i in range(10):
            a.train_classes[i] = int(i in trained)
        a.w_weak, a.w_fit, a.fit_only_2d, a.B = w_weak, 1.0, only2d, B
        a.d_dims, a.dout9, a.fit_prob = fptr(b.out('d_dims', (B, 3))), fptr(b.out('dout9', (B, 9))), fptr(b.out('fit_prob', B))
        a.terms, a.loss = fptr(b.out('terms', 2)), fptr(b.out('loss', 1))
        a._keep = b
        return a
    tag = 'semi_final_loss B=%d only2d=%d %s ' % (B, only2d, variant)
    got, ref = both(env, 't3d_semi_final_loss', build, tag)
    for k, shape in (('d_dims', (B, 3)), ('dout9', (B, 9)), ('fit_prob', B), ('terms', 2), ('loss', 1)):
        _close(tag + k, val(got, k, shape), val(ref, k, shape), 1e-5, 1e-6)          # test_stage_c_glue_kernels
    gd = val(got, 'd_dims', (B, 3))
    if variant != 'default':
        assert not gd.any() and float(val(got, 'terms', 2)[0]) == 0.0
    elif B >= 7:
        assert not gd[3].any(), 'the single member of class 6 sits on its class mean'
        assert 8 not in d['cls'] and (d['cls'] == 6).sum() == 1
        assert gd[4].any() and gd[5].any(), 'the soft row is a member of class 2 (the first of its two largest entries)'
    assert not val(got, 'dout9', (B, 9))[:, :7].any()


ANCHOR_B = [1, 32, 1024]


def check_anchor_reg_bwd(env, B, ld_box, with7, with_dd):
    r = np.random.RandomState(500 + B)
    box = r.normal(size=(B, 67)).astype(F32)
    box[0, 37:67] = -1.5                                       # raw <= 1e-5 in every class: the max() clamp kills that gradient
    if B > 2:
        box[2, 27:37] = 0.0
        box[2, 27 + 4], box[2, 37 + 12:37 + 15] = 9.0, -1.0    # raw = mean - mean = 0 exactly: clamped as well
        box[1, 3:15], box[1, 27:37] = box[1, 3:15] * 0.1, box[1, 27:37] * 0.1
        box[1, 3 + 4] = box[1, 3 + 9] = 2.0                    # ties: the first arg-max takes the gradient
        box[1, 27 + 0] = box[1, 27 + 6] = 2.0
    dbox7, dd = r.normal(size=(B, 7)).astype(F32), r.normal(size=(B, 3)).astype(F32)
    g0, s0 = r.normal(size=(B, 67)).astype(F32), r.normal(size=(B, 3)).astype(F32)

    def build(b):
        a = abi.AnchorRegBwdArgs(fptr(b.inp(nan_cols(box, ld_box))), ld_box, fptr(b.inp(dbox7) if with7 else None),
                                 fptr(b.inp(dd) if with_dd else None), fptr(b.out('dbox', (B, 67), init=g0)), fptr(b.out('dstage1', (B, 3), init=s0)), B)
        a._keep = b
        return a
    tag = 'anchor_reg_bwd B=%d ld=%d dbox7=%d d_dims=%d ' % (B, ld_box, with7, with_dd)
    got, ref = both(env, 't3d_anchor_reg_bwd', build, tag)
    g, rg = val(got, 'dbox', (B, 67)), val(ref, 'dbox', (B, 67))
    _close(tag + 'dbox', g, rg, 1e-5, 1e-6)                    # test_stage_c_glue_kernels
    _close(tag + 'dstage1', val(got, 'dstage1', (B, 3)), val(ref, 'dstage1', (B, 3)), 1e-6, 1e-6)
    # accumulation: what the spec leaves at its pre-filled bits keeps them in the library's output too
    for k, init in (('dbox', g0), ('dstage1', s0)):
        same = val(ref, k, init.shape, np.int32) == init.view(np.int32)
        assert k != 'dbox' or same.mean() > 0.8              # (at most 7 of a row's 67 entries are picked)
        assert (val(got, k, init.shape, np.int32)[same] == init.view(np.int32)[same]).all(), tag + k + ': an entry outside the picked bins moved'
    if not with7 and not with_dd:
        assert (val(got, 'dbox', (B, 67), np.int32) == g0.view(np.int32)).all()
    if with7 or with_dd:
        assert (g[0, 37:67] == g0[0, 37:67]).all(), 'a clamped size took a gradient'
        if B > 2:
            assert (g[2, 37:67] == g0[2, 37:67]).all() and (g[1, 37 + 18:37 + 21] == g0[1, 37 + 18:37 + 21]).all()
            assert (g[1, 37:40] != g0[1, 37:40]).all()
    if with7 and B > 2:
        assert g[1, 15 + 4] != g0[1, 15 + 4] and g[1, 15 + 9] == g0[1, 15 + 9]


def check_anchor_reg_bwd_refusals(env):
    for B, ld in ((32, 66), (0, 67), (1025, 67)):
        b = Bufs(env.dev)
        z = b.inp(np.zeros((1025, 67), F32))
        a = abi.AnchorRegBwdArgs(fptr(z), ld, fptr(z), fptr(z), fptr(b.out('dbox', (32, 67))), fptr(b.out('dstage1', (32, 3))), B)
        assert call(env, 't3d_anchor_reg_bwd', a) == ERR_SHAPE, (B, ld)
        env.sync()
        snap = b.snapshot()
        assert (words(snap, 'dbox') == SENT).all() and (words(snap, 'dstage1') == SENT).all()


# ======================================================================================================================================
# 3. t3d_seg_head / t3d_seg_finalize
# ======================================================================================================================================
SEG_SHAPES = [(1, 128, 3), (3, 256, 4), (2, 1024, 7)]          # B, rows_per_frustum, ld_pc
SEG_FORMS = ['infer', 'labels', 'train_nodrop', 'train_mask', 'train_gen', 'dsoft', 'oracle', 'oracle_dz', 'ties']
SEG_K = 128
GAMMA_136 = 136 * 2.0 ** -24 / (1 - 136 * 2.0 ** -24)          # the fp32 dot product of 128 terms, the bias and the element-wise chain in front
DROP_SEED, DROP_STEP, KEEP = 4321, 7, 0.5


def _seg_d(y, sc, sh, keep):
    return np.maximum(y.astype(np.float64) * sc + sh, 0) * keep


def seg_margin(y, sc, sh, keep, w, bias):
    """(|q0 - q1| of the spec, the fp32 dot-product bound gamma_136 sum_k |d_k| (|w_k0| + |w_k1|)) per row."""
    d = _seg_d(y, sc, sh, keep)
    q = d @ w.astype(np.float64) + bias
    return np.abs(q[:, 0] - q[:, 1]), GAMMA_136 * (np.abs(d) @ np.abs(w.astype(np.float64)).sum(1))


def seg_inputs(B, rpf, form, seed=9):
    """_seg_inputs, as a copy of the cached case (no caller can change it for the next)."""
    return {k: v.copy() for k, v in _seg_inputs(B, rpf, form, seed).items()}


@functools.lru_cache(maxsize=None)
def _seg_inputs(B, rpf, form, seed):
    """Inputs of one seg-head case.  Every row's |q0 - q1| is at least 4 x its own fp32 dot-product bound (rows that fail are redrawn),
    so the hard mask, the masked sums and the accuracy count of an fp32 kernel are those of the fp64 spec: nothing is left out of the
    comparison.  y is bf16-representable (the bf16 kernel reads the same numbers); the xyz are multiples of 1/64 below 4 in magnitude
    (any order of the 128-row sums is exact)."""
    r = np.random.RandomState(seed + 7 * B + rpf)
    M, K = B * rpf, SEG_K
    sc, sh = (0.5 + r.uniform(size=K)).astype(F32), (r.normal(size=K) * 0.3).astype(F32)
    w = (r.normal(size=(K, 2)) * 0.2).astype(F32)
    bias = np.array([0.1, 0.1] if form == 'ties' else [0.1, -0.2], F32)
    dm = (r.uniform(size=(M, K)) < KEEP).astype(F32)
    keep = np.ones((M, K))
    if form == 'train_mask':
        keep = dm.astype(np.float64) / KEEP
    elif form == 'train_gen':
        keep = hash_keep_mask(DROP_SEED, DROP_STEP, M * K, KEEP).reshape(M, K).astype(np.float64) / KEEP
    draw = lambda n: _bf16_values(r.normal(size=(n, K)).astype(F32))
    y = draw(M)
    tie_rows = np.arange(3, M, 37) if form == 'ties' else np.zeros(0, np.int64)
    y[tie_rows] = -8.0                                        # scale > 0 and |shift| ~ 0.3: every activation <= 0, both logits the bias
    for _ in range(50):
        gap, bound = seg_margin(y, sc, sh, keep, w, bias)
        bad = np.nonzero(gap < 4 * bound)[0]
        if len(bad) == 0:
            break
        y[bad] = draw(len(bad))
    d = dict(y=y, sc=sc, sh=sh, w=w, bias=bias, dm=dm, keep=keep, tie_rows=tie_rows,
             lab=(r.uniform(size=M) < 0.3).astype(np.int32), is2d=(np.arange(B) % 2).astype(np.int32) if B > 1 else np.zeros(1, np.int32),
             pc=(r.randint(-255, 256, size=(M, 7)) / 64.0).astype(F32), dsoft=(r.normal(size=M) * 1e-3).astype(F32),
             om=(r.uniform(size=M) < 0.4).astype(np.int32))
    return d


def check_seg_margin(B, rpf, form):
    d = seg_inputs(B, rpf, form)
    gap, bound = seg_margin(d['y'], d['sc'], d['sh'], d['keep'], d['w'], d['bias'])
    assert (gap >= 4 * bound).all(), (B, rpf, form, int((gap < 4 * bound).sum()))
    assert np.array_equal(_bf16_values(d['y']), d['y'])
    if form == 'ties':
        assert len(d['tie_rows']) > 0 and (gap[d['tie_rows']] == 0).all() and (bound[d['tie_rows']] == 0).all()
        assert (gap[np.setdiff1d(np.arange(B * rpf), d['tie_rows'])] > 0).all()


def seg_head_build(d, B, rpf, ld_pc, form, bf16, ce_weight=0.37):
    M, K, T = B * rpf, SEG_K, B * rpf // 128

    def build(b):
        as16 = bf16 and b.dev.type != 'cpu'                 # the spec reads the same values as fp32 and stores dz as fp32
        a = abi.SegHeadArgs()
        y = b.inp(d['y'])
        if as16:
            y = y.bfloat16()
            b.keep.append(y)
        a.y, a.scale, a.shift, a.dtype = fptr(y), fptr(b.inp(d['sc'])), fptr(b.inp(d['sh'])), abi.BF16 if as16 else abi.F32
        a.keep_prob = 1.0
        if form == 'train_mask':
            a.drop_mask, a.keep_prob = fptr(b.inp(d['dm'])), KEEP
        elif form == 'train_gen':
            a.drop_seed, a.drop_hyper, a.keep_prob = DROP_SEED, fptr(b.inp(np.array([DROP_STEP, 0, 0, 0], F32))), KEEP
        a.w, a.bias, a.pc, a.ld_pc, a.ce_weight = fptr(b.inp(d['w'])), fptr(b.inp(d['bias'])), fptr(b.inp(np.ascontiguousarray(d['pc'][:, :ld_pc]))), ld_pc, ce_weight
        if form != 'infer':
            a.labels, a.is_data_2D = iptr(b.inp(d['lab'])), iptr(b.inp(d['is2d']))
        if form in ('oracle', 'oracle_dz'):
            a.oracle_mask = iptr(b.inp(d['om']))
        if form not in ('infer', 'labels', 'oracle'):
            a.dz = fptr(b.out('dz', (M, K), dtype=torch.bfloat16 if as16 else torch.float32))
            a.psum_dz, a.psum_dzy, a.dw_part = fptr(b.out('psum_dz', (T, K))), fptr(b.out('psum_dzy', (T, K))), fptr(b.out('dw_part', (T, K, 2)))
        if form == 'dsoft':
            a.dsoft = fptr(b.inp(d['dsoft']))
        a.logits, a.mask, a.part = fptr(b.out('logits', (M, 2))), fptr(b.out('mask', M)), fptr(b.out('part', (T, 8)))
        a.M, a.K, a.rows_per_frustum, a.B = M, K, rpf, B
        a._keep = b
        return a
    return build


def compare_seg_head(tag, got, ref, d, B, rpf, form, as16):
    """Tolerances of test_seg_head_and_finalize; the hard mask, part[:, 1:5] and part[:, 7] exactly."""
    M, K, T = B * rpf, SEG_K, B * rpf // 128
    _close(tag + 'logits', val(got, 'logits', (M, 2)), val(ref, 'logits', (M, 2)), 1e-5, 2e-5)
    mask, part, rpart = val(got, 'mask', M), val(got, 'part', (T, 8)), val(ref, 'part', (T, 8))
    assert np.array_equal(mask, val(ref, 'mask', M)), tag + 'hard mask'
    assert np.array_equal(part[:, 1:5], rpart[:, 1:5]), tag + 'part[:, 1:5]'
    assert np.array_equal(part[:, 7], rpart[:, 7]), tag + 'part[:, 7] (n_correct)'
    _close(tag + 'part[:, 0|5|6]', part[:, [0, 5, 6]], rpart[:, [0, 5, 6]], 1e-4, 1e-3)
    if form == 'ties':
        t = d['tie_rows']
        lg = val(got, 'logits', (M, 2))
        assert (lg[t] == d['bias']).all() and not mask[t].any()
        tiles = np.unique(t // 128)
        assert (rpart[tiles, 7] > 0).any()
    if form in ('oracle', 'oracle_dz'):
        om = d['om'].astype(F32)
        assert np.array_equal(val(got, 'logits', (M, 2)), np.stack([1 - om, om], 1)) and np.array_equal(mask, om)
    if 'dz' not in got:
        assert form in ('infer', 'labels', 'oracle')
        return
    rdz = val(ref, 'dz', (M, K)).astype(np.float64)
    if as16:
        dz = torch.as_tensor(val(got, 'dz', (M, K), np.int16).copy()).view(torch.bfloat16).float().numpy().astype(np.float64)
        # the stored bf16 value: half a bf16 spacing (2^-8 |ref|; a rounding flip stays inside it) on top of the f32 case's bound
        _within(tag + 'dz (bf16)', dz, rdz, 2.0 ** -8 * np.abs(rdz) + 1e-4 * np.abs(rdz) + 1e-8)
        # "the partial sums are those of the gradient as stored" (k_seg_head): against sums of the stored dz
        y3 = d['y'].astype(np.float64).reshape(T, 128, K)
        s1, s2 = dz.reshape(T, 128, K).sum(1), (dz.reshape(T, 128, K) * y3).sum(1)
    else:
        dz = val(got, 'dz', (M, K)).astype(np.float64)
        _close(tag + 'dz', dz, rdz, 1e-4, 1e-8)
        s1, s2 = val(ref, 'psum_dz', (T, K)), val(ref, 'psum_dzy', (T, K))
    _close(tag + 'psum_dz', val(got, 'psum_dz', (T, K)), s1, 1e-3, 1e-6)
    _close(tag + 'psum_dzy', val(got, 'psum_dzy', (T, K)), s2, 1e-3, 1e-6)
    _close(tag + 'dw_part', val(got, 'dw_part', (T, K, 2)), val(ref, 'dw_part', (T, K, 2)), 1e-3, 1e-6)
    if form == 'oracle_dz':
        assert not dz.any() and not val(got, 'dw_part', (T, K, 2)).any()
    else:
        assert np.abs(rdz).max() > 0


def check_seg_head(env, B, rpf, ld_pc, form, bf16):
    d = seg_inputs(B, rpf, form)
    tag = 'seg_head B=%d rpf=%d ld_pc=%d %s %s ' % (B, rpf, ld_pc, form, 'bf16' if bf16 else 'f32')
    got, ref = both(env, 't3d_seg_head', seg_head_build(d, B, rpf, ld_pc, form, bf16), tag)
    compare_seg_head(tag, got, ref, d, B, rpf, form, bf16 and env.dev.type != 'cpu')


FINALIZE_SHAPES = [(1, 1), (3, 2), (257, 1), (300, 3), (40, 16)]          # B, tiles_per_frustum: the stride-256 loops over B and over T = 900, 640


def check_seg_finalize(env, B, tpf, given):
    r = np.random.RandomState(600 + B + tpf)
    T, K, rpf = B * tpf, SEG_K, 128 * tpf
    part = r.normal(size=(T, 8)).astype(F32)
    part[:, 0] = np.abs(part[:, 0]) * 40
    part[:, 1] = r.randint(0, 129, size=T)
    part[:, 7] = r.randint(0, 129, size=T)
    zero_b = B // 2
    part[zero_b * tpf:(zero_b + 1) * tpf, 1] = 0               # a frustum with an empty mask: den = 1
    dwp = r.normal(size=(T, K, 2)).astype(F32)
    outs = [('mask_xyz_mean', (B, 3))] + [(k, s) for k, s in (('seg_loss', B), ('dw', (K, 2)), ('dbias', 2), ('n_correct', 1)) if given]

    def build(b):
        a = abi.SegFinalizeArgs()
        a.part, a.B, a.tiles_per_frustum, a.rows_per_frustum, a.K = fptr(b.inp(part)), B, tpf, rpf, K
        a.dw_part = fptr(b.inp(dwp))
        for k, shape in outs:
            setattr(a, k, fptr(b.out(k, shape)))
        a._keep = b
        return a
    tag = 'seg_finalize B=%d tpf=%d given=%d ' % (B, tpf, given)
    got, ref = both(env, 't3d_seg_finalize', build, tag)
    assert sorted(got) == sorted(k for k, _ in outs)
    for k, shape in outs:
        _close(tag + k, val(got, k, shape), val(ref, k, shape), 1e-5, 1e-6)          # test_seg_head_and_finalize
    s = part.astype(np.float64).reshape(B, tpf, 8).sum(1)
    _within(tag + 'mean of the empty frustum', val(got, 'mask_xyz_mean', (B, 3))[zero_b], s[zero_b, 2:5], 1e-5 * np.abs(s[zero_b, 2:5]) + 1e-6)
    if given:
        assert float(val(got, 'n_correct', 1)[0]) == part[:, 7].astype(np.float64).sum()


# ======================================================================================================================================
# 4. optimiser and element-wise kernels
# ======================================================================================================================================
# (n_slabs, numel, slab misalignment): all three slab loops of the float4 path alone and chained (1, 8: the 8-slab tail; 25, 33: the 32-slab loop
# [+ tail]; 57, 65, 130: the 64-slab loop [+ 32 + tail]), the scalar path (67, 1023; a multiple-of-4 numel behind a slab_off that is no
# multiple of 4), one tensor of 40 004 elements (10 001 float4 > 256 x 32: the grid cap and the stride loop)
SLAB_TABLE = [(1, 4, 0), (8, 640, 0), (9, 67, 0), (25, 1023, 0), (33, 640, 0), (57, 640, 0), (65, 4, 0), (130, 640, 0), (57, 67, 0), (65, 1023, 0),
              (9, 40004, 0), (33, 640, 2), (130, 1023, 0)]


def check_reduce_slabs(env, max_numel):
    r = np.random.RandomState(700)
    n_t = len(SLAB_TABLE)
    table = (abi.SlabDesc * n_t)()
    so, go = 0, 8
    for i, (ns, ne, mis) in enumerate(SLAB_TABLE):
        so += (-so) % 4 + mis
        table[i] = abi.SlabDesc(so, go, ne, ns)
        so += ns * ne
        go += ne + 4                                         # four untouched elements between two gradient regions
        go += (-go) % 4
    slab = r.normal(size=so).astype(F32)
    assert all(table[i].slab_off % 4 == SLAB_TABLE[i][2] and table[i].grad_off % 4 == 0 for i in range(n_t))
    b = Bufs(env.dev)
    sl, grad = b.inp(slab), b.out('grad', go)
    assert sl.data_ptr() % 16 == 0
    if env.dev.type == 'cpu':
        tab = table
    else:
        tab_dev = b.inp(np.frombuffer(bytes(table), dtype=np.uint8).copy())
        tab = C.cast(C.c_void_p(tab_dev.data_ptr()), C.POINTER(abi.SlabDesc))
    assert env.lib.t3d_reduce_slabs(fptr(sl), fptr(grad), tab, n_t, max_numel, env.stream()) == 0
    env.sync()
    snap = b.snapshot()
    rc.check_guards(snap, 'reduce_slabs')
    g, gw = val(snap, 'grad', go), val(snap, 'grad', go, np.int32)
    live, failed = np.zeros(go, bool), []
    for i, (ns, ne, mis) in enumerate(SLAB_TABLE):
        d = table[i]
        s = slab[d.slab_off:d.slab_off + ns * ne].astype(np.float64).reshape(ns, ne)
        live[d.grad_off:d.grad_off + ne] = True
        # any order of ns fp32 additions: every partial sum is at most sum|slab| of its element, every addition rounds at 2^-24 of it
        try:
            _within('reduce_slabs max_numel=%d slabs=%d numel=%d mis=%d' % (max_numel, ns, ne, mis), g[d.grad_off:d.grad_off + ne], s.sum(0),
                    ns * 2.0 ** -24 * np.abs(s).sum(0))
        except AssertionError as e:                            # (every tensor of the table is looked at: the message names each one that fails)
            failed.append(str(e))
    assert not failed, failed
    assert (gw[~live] == SENT).all(), 'reduce_slabs wrote between the gradient regions'


OPT_N = [1, 255, 257, 2048 * 256 + 3]          # the last: three elements behind the 2048-block grid cap (the grid-stride trip)
SCHED = (1e-3, 0.5, 800000.0, 0.5, 0.5, 400000.0, 0.99, 0.9, 0.999, 32, 1)          # step_offset 1: the call runs step hyper[0] + 1 and leaves hyper[0] + 2


def _hyper(b, start):
    return b.inp(np.array([start, 0, 0, 0], F32))


def check_adam_and_momentum(env, n):
    r = np.random.RandomState(800 + n % 1000)
    w0, g0 = r.normal(size=n).astype(F32), (r.normal(size=n) * 1e-2).astype(F32)
    sched = abi.Schedule(*SCHED)

    def run(e):
        b = Bufs(e.dev)
        z = np.zeros(n, F32)
        h, g = _hyper(b, 0.0), b.inp(g0)
        w, m, v = b.out('w', n, init=w0), b.out('m', n, init=z), b.out('v', n, init=z)
        wm, acc = b.out('wm', n, init=w0), b.out('acc', n, init=z)
        for _ in range(3):
            assert e.lib.t3d_schedule_step(fptr(h), C.byref(sched), e.stream()) == 0
            assert e.lib.t3d_adam_tf_step(fptr(w), fptr(g), fptr(m), fptr(v), n, fptr(h), 0.9, 0.999, 1e-8, 0.5, e.stream()) == 0
            assert e.lib.t3d_momentum_step(fptr(wm), fptr(g), fptr(acc), n, fptr(h), 0.9, 0.5, e.stream()) == 0
        e.sync()
        return b.snapshot()
    ref, got = run(SPEC), run(env)
    rc.check_guards(got, 'adam / momentum n=%d' % n)
    tag = 'optimiser n=%d ' % n
    # test_reduce_slabs_adam_schedule_dropout: w 1e-6 / 1e-7, v 1e-4 / 1e-12, momentum w 1e-6 / 1e-7, accumulator 1e-6 / 1e-9; m as the accumulator
    for k, rtol, atol in (('w', 1e-6, 1e-7), ('v', 1e-4, 1e-12), ('m', 1e-6, 1e-9), ('wm', 1e-6, 1e-7), ('acc', 1e-6, 1e-9)):
        _close(tag + k, val(got, k, n), val(ref, k, n), rtol, atol)
    assert (g0 != 0).all() and val(got, 'm', n).all() and val(got, 'v', n).all() and val(got, 'acc', n).all(), 'an element was not visited'


MASK_N = [1, 257, 4096 * 256 + 77]             # the last: 77 elements behind the 4096-block grid cap


def check_dropout_mask(env, n):
    for keep in (0.5, 1.0, 1e-3):
        for step in (0, 7, 2 ** 24):
            for seed in (0x80000001, 1234):
                if seed == 1234 and (keep != 0.5 or step != 7):
                    continue
                b = Bufs(env.dev)
                mask = b.out('mask', n)
                assert env.lib.t3d_dropout_mask(fptr(mask), n, keep, seed, fptr(_hyper(b, float(step))), env.stream()) == 0
                env.sync()
                snap = b.snapshot()
                rc.check_guards(snap, 'dropout_mask')
                want = hash_keep_mask(seed, step, n, keep)
                _same_bits('dropout_mask n=%d keep=%g step=%d seed=%#x' % (n, keep, step, seed), torch.as_tensor(val(snap, 'mask', n).copy()), torch.as_tensor(want))
                assert keep < 1.0 or want.all()
                if keep == 0.5 and n > 4096 * 256:             # both values occur behind the grid cap: the stride trip is looked at
                    assert 0 < want[4096 * 256:].sum() < n - 4096 * 256


CAST_N = [1, 7, 8, 9, 2047, 2049, 2048 * 2048 + 5]          # the vector body, the scalar tail, the grid-stride loop (2048 blocks x 2048 elements)
# exact round-to-even ties (down to 1.0, up to 1.015625, the negative ones), denormals, +-inf, the largest finite fp32 (rounds to inf), NaN
CAST_SPECIALS = np.array([1.00390625, 1.01171875, -1.00390625, -1.01171875, 1e-40, -1e-45, np.inf, -np.inf, 3.4028235e38, -3.4028235e38, np.nan,
                          0.0, -0.0, 1.0039063, 1.0039062], F32)


def cast_input(n):
    r = np.random.RandomState(900 + n % 1000)
    x = (r.normal(size=n) * np.exp(r.uniform(-20, 20, size=n))).astype(F32)
    k = min(n, len(CAST_SPECIALS))
    x[:k] = CAST_SPECIALS[:k]
    if n > 64:
        x[-len(CAST_SPECIALS):] = CAST_SPECIALS          # in the scalar tail / the last grid-stride trip too
    return x


def check_cast_bf16(env, n):
    x = cast_input(n)
    b = Bufs(env.dev)
    src, dst = b.inp(x), b.out('dst', n, dtype=torch.bfloat16)
    assert src.data_ptr() % 16 == 0
    assert env.lib.t3d_cast_bf16(fptr(src), C.c_void_p(dst.data_ptr()), n, env.stream()) == 0
    env.sync()
    snap = b.snapshot()
    rc.check_guards(snap, 'cast_bf16 n=%d' % n)
    half = rc.body(snap, 'dst', np.int16)
    got = torch.as_tensor(half[:n].copy()).view(torch.bfloat16)
    want = torch.as_tensor(x).to(torch.bfloat16)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), 'NaN compares as NaN'
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]), 'cast_bf16 n=%d: not the bits of torch.Tensor.to(bfloat16)' % n
    assert np.array_equal(half[n:], np.full(len(half) // 2, SENT, np.int32).view(np.int16)[n:]), 'the half word behind an odd n was written'


def check_cast_bf16_refusals(env):
    b = Bufs(env.dev)
    src, dst = b.inp(np.ones(64, F32)), b.out('dst', 64, dtype=torch.bfloat16)
    for so, do in ((4, 0), (0, 2), (0, 8), (8, 8)):
        assert env.lib.t3d_cast_bf16(C.cast(C.c_void_p(src.data_ptr() + so), abi.F), C.c_void_p(dst.data_ptr() + do), 16, env.stream()) == ERR_ARG, (so, do)
    env.sync()
    assert (words(b.snapshot(), 'dst') == SENT).all()


def check_schedule_step(env):
    """Four calls around each staircase with step_offset = 1 (the pipelined step's second context): the calls run steps start + 1, + 3,
    + 5, + 7.  lr halves from step 25 000 on (25 000 x 32 = 800 000 samples), the bn momentum term from step 12 500 on (400 000): from
    24 996 / 12 496 the calls step over the staircase step (24 999 -> 25 001), from 24 997 / 12 497 the second call runs it exactly."""
    sched = abi.Schedule(*SCHED)
    for start, edge, col in ((24996, 25000, 1), (24997, 25000, 1), (12496, 12500, 2), (12497, 12500, 2)):
        hs = []
        for e in (SPEC, env):
            b = Bufs(e.dev)
            h = b.out('hyper', 4, init=np.array([start, 0, 0, 0], F32))
            trace = []
            for _ in range(4):
                assert e.lib.t3d_schedule_step(fptr(h), C.byref(sched), e.stream()) == 0
                e.sync()
                snap = b.snapshot()
                trace.append(val(snap, 'hyper', 4).copy())
            rc.check_guards(snap, 'schedule_step')
            hs.append(np.stack(trace))
        _close('schedule_step from %d' % start, hs[1], hs[0], 1e-6, 1e-9)          # test_reduce_slabs_adam_schedule_dropout's 'hyper'
        late = np.array([start + 1 + 2 * i >= edge for i in range(4)])          # the calls that run a step at or behind the staircase
        assert late.any() and not late.all() and any(start + 1 + 2 * i == edge for i in range(4)) == bool(start % 2)
        for tr in hs:
            v = tr[:, col]
            assert (v[~late] == v[0]).all() and (v[late] == v[-1]).all() and v[0] != v[-1], ('staircase', start, v)
        assert (hs[1][:, 0] == start + 2 * np.arange(1, 5)).all()


# ======================================================================================================================================
# 5. t3d_weak_loss shapes
# ======================================================================================================================================
WEAK_SHAPES = [(1, 128), (65, 128), (256, 128), (4, 2048)]
WEAK_FORMS = ['both', 'no_is2d', 'pc_only', 'rtilt_only', 'no_total']


def weak_build(d, B, N, form):
    """The default switch set of test_weak_loss_values_and_gradients (models/config.py) and its weights."""
    M, ldpc = B * N, 4
    surf, rep = form != 'rtilt_only', form != 'pc_only'
    pc4 = np.zeros((M, ldpc), F32)
    pc4[:, :3] = d['pc'].reshape(M, 3)

    def build(b):
        a = abi.WeakLossArgs()
        a.center, a.reg_dims, a.reg_theta = fptr(b.inp(d['center'])), fptr(b.inp(d['dims'])), fptr(b.inp(d['theta']))
        if surf:
            a.pc, a.ld_pc, a.logits = fptr(b.inp(pc4)), ldpc, fptr(b.inp(d['logits']))
            a.surf_part, a.dsoft, a.surface = fptr(b.out('surf_part', (B, N // 128, 8), init=np.zeros((B, N // 128, 8), F32))), fptr(b.out('dsoft', M)), fptr(b.out('surface', B))
        if rep:
            a.Rtilt, a.K, a.rot_frust, a.box2D = fptr(b.inp(d['Rtilt'])), fptr(b.inp(d['K'])), fptr(b.inp(d['rot_frust'])), fptr(b.inp(d['box2D']))
            a.img_dim, a.reproj = fptr(b.inp(d['img_dim'])), fptr(b.out('reproj', B))
        if form != 'no_is2d':
            a.is_data_2D = iptr(b.inp(d['is2d']))
        a.w_reproj, a.w_surface, a.multiplier = (0.01 if rep else 0.0), (1.0 if surf else 0.0), 0.5
        a.use_softmax_proj, a.softmax_scale, a.dilate, a.clip_lower_b_loss, a.clip_pred_box, a.loss_mse = 0, 10.0, 1.5, 1, 0, 0
        a.train_box_reproj, a.train_box_surface = (C.c_int32 * 3)(1, 1, 1), (C.c_int32 * 3)(1, 0, 1)
        a.surface_margin, a.surface_scale_dims = 0.05, 0.9
        a.dbox7 = fptr(b.out('dbox7', (B, 7)))
        if form != 'no_total':
            a.total_losses = fptr(b.out('total_losses', B, init=np.full(B, 0.25, F32)))
        a.loss, a.B, a.N = fptr(b.out('loss', 1, init=np.full(1, 3.0, F32))), B, N
        a._keep = b
        return a
    return build


def check_weak_loss(env, B, N, form):
    from test_weak_gpu import camera_case
    d = camera_case(B, N, seed=3)
    tag = 'weak_loss B=%d N=%d %s ' % (B, N, form)
    got, ref = both(env, 't3d_weak_loss', weak_build(d, B, N, form), tag)

    def close(k, shape, rel, shift=0.0):
        # test_weak_loss_values_and_gradients: |error| <= rel * max(1e-6, max|ref|)
        r = val(ref, k, shape).astype(np.float64) - shift
        _within(tag + k, val(got, k, shape).astype(np.float64) - shift, r, rel * max(1e-6, float(np.abs(r).max())))
    if 'reproj' in got:
        close('reproj', B, 2e-4)
    if 'surface' in got:
        close('surface', B, 2e-5)
        close('dsoft', B * N, 2e-5)
    if 'total_losses' in got:
        close('total_losses', B, 2e-4, 0.25)
    close('loss', 1, 2e-4, 3.0)
    close('dbox7', (B, 7), 5e-4)
    assert ('reproj' in got) == (form != 'pc_only') and ('surface' in got) == (form != 'rtilt_only') and ('total_losses' in got) == (form != 'no_total')
    assert float(np.abs(val(ref, 'dbox7', (B, 7))).max()) > 0 or (B == 1 and form != 'no_is2d')


def check_weak_loss_refusals(env):
    from test_weak_gpu import camera_case
    for B, N in ((257, 128), (4, 192)):
        d = camera_case(B, 256 if N % 128 else N, seed=3)
        code, snap = launch(env, 't3d_weak_loss', weak_build(d, B, N, 'rtilt_only') if N % 128 == 0 else _weak_bad_n(d, B, N))
        assert code == ERR_SHAPE, (B, N)
        assert (words(snap, 'dbox7') == SENT).all()


def _weak_bad_n(d, B, N):
    inner = weak_build(d, B, 256, 'both')

    def build(b):
        a = inner(b)
        a.N = N
        return a
    return build


# ======================================================================================================================================
# form coverage: forms_text() is the table in the docstring of tests/test_kernels_heads_gpu.py (tests/test_kernels_heads_cpu.py holds the two together)
# ======================================================================================================================================
FORMS = [
    ('k_strong_loss<true> (B <= 128: heads and gradients in LDS; summary on thread 512 + f)', 'test_strong_loss[1-*], [128-*], test_strong_loss_argument_branches[64-*]'),
    ('k_strong_loss<false>, 128 < B <= 512 (private gradient, summary on thread 512 + f)', 'test_strong_loss[129-*], [512-*], test_strong_loss_argument_branches[129-*]'),
    ('k_strong_loss<false>, B > 512 (summary inline)', 'test_strong_loss[513-*], [1024-*]'),
    ('k_strong_loss without IoU outputs / without seg_loss / normalize_by_3d_count / ld_box 72', 'test_strong_loss[*-short], test_strong_loss_argument_branches'),
    ('k_strong_loss all-2-D batch (1e-3 guard)', 'test_strong_loss_all_2d_batch'),
    ('k_box_head_iou: one 64-thread block, a partial block, several blocks; stage1_center NULL', 'test_box_head_iou'),
    ('k_dgrad_narrow: one / two / three column chunks, one / both accumulators, fp32 and bf16 dy', 'test_dgrad_narrow'),
    ('k_semi_final_loss: B below the class count, one full workgroup, T = 0, w_weak = 0, empty / single-member class, soft tie', 'test_semi_final_loss'),
    ('k_anchor_reg_bwd: optional pointers, accumulation, clamp, ties, ld_box 72', 'test_anchor_reg_bwd'),
    ('k_seg_head<float> / <bf16_t>: infer, labels, train (no dropout, stored mask, generated mask), oracle_mask, exact ties', 'test_seg_head'),
    ('k_seg_head<float, true> / <bf16_t, true> (dsoft)', 'test_seg_head[*-dsoft-*]'),
    ('k_seg_finalize: stride-256 loops over frustums (257, 300) and tiles (900, 640), empty mask, optional outputs', 'test_seg_finalize'),
    ('reduce_slabs_body: 8-, 32- and 64-slab loops alone and chained, scalar path, misaligned slab_off, grid cap 256, small max_numel', 'test_reduce_slabs'),
    ('k_adam_tf / k_momentum_tf: one thread, part of a block, two blocks, the 2048-block cap', 'test_adam_and_momentum'),
    ('k_dropout_mask: the 4096-block cap, keep 1 and 1e-3, step 2^24, seed with the top bit', 'test_dropout_mask'),
    ('k_cast_bf16: vector body, scalar tail, grid-stride loop, alignment refusal', 'test_cast_bf16, test_cast_bf16_refusals'),
    ('k_schedule_step: both staircases, step_offset', 'test_schedule_step'),
    ('k_weak_surface / k_weak_finish: B = 1, 65, 256 (tot[256] full), 16 tiles per frustum, optional inputs', 'test_weak_loss'),
]


def forms_text():
    return '\n'.join('  %-130s %s' % f for f in FORMS)
