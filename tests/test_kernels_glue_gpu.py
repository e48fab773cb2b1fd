"""GPU: the Box-PC, refinement and glue entry points of libt3d.so that tests/test_kernels_gpu.py does not call through the C ABI --
t3d_box_refine_step_bwd, t3d_boxpc_rep_b, t3d_box2d_feats, t3d_act_dropout, t3d_pool_bwd_mid -- and the argument branches it leaves
out of t3d_box_refine_step (weigh_by_conf = 2, fit_prob = NULL), t3d_boxpc_rep (rowmask), t3d_boxpc_rep_bwd (rows_per_frustum other
than 256) and t3d_boxpc_loss (weigh_pred_by_cls_conf, grad_cls_via_delta, delta_loss_mse): each against the NumPy fp64 specification
(tests/fake_t3d.py, tests/ref_boxpc_b.py) on identical seeded fp32 inputs, called through ctypes with the abi.py structs.

The bounds are derived (they are written where they are used) or are those of the neighbouring tests of test_kernels_gpu.py; none is
measured.  Every test prints its worst error next to the bound that applied there.

`1 - p_fit` in both refinement kernels is formed in fp32, as the reference's graph forms it (test_semisup.py:116-121: weight =
1 - softmax(fit logits)[:, 1] on float32 tensors), so the weight w = (1 - p)^n carries an ABSOLUTE error of a few 2^-24 however small
it is: not a bug, and the reason for the 2^-22 terms below.

MEASURED_WORST (one run of this module on the MI355X, 101 passed; per output, over its cases: the largest `worst` that `_within`
prints, the bound at that element, and the largest `largest error / bound`):
  refine_step_bwd tot_out                    0          (1.745e-06)  0.000   also with out9 = NULL and in place; dout9 untouched
  refine_step_bwd dout9[:, :7]               4.768e-07  (4.856e-05)  0.194   B=300 n=1 via=1 carry=1
  refine_step_bwd dout9[:, 7:9]              4.768e-07  (3.913e-05)  0.023   B=300 n=2 via=1 carry=1; columns 7 and 8 negations bit for bit
  refine_step c / s                          2.384e-07 / 2.384e-07  (2.328e-05 / 2.887e-05)  0.057 / 0.029
  refine_step th / tot                       2.384e-07 / 2.384e-07  (2.657e-05 / 2.932e-05)  0.028 / 0.027
  refine_step fit_prob                       5.960e-08  (9.432e-06)  0.009
  rep_b box_out                              0          (1.603e-06)  0.000   bit for bit t3d_boxpc_rep's; pc_out bit for bit the spec's fp32
  rep rowmask rep / box                      9.537e-07 / 0  (3.137e-05 / 1.492e-06)  0.059 / 0.000   rep[:, :C] bit for bit rep_b's pc_out
  rep_bwd dbox                               1.788e-07  (6.973e-05)  0.009   rpf=256 C=3 coff=2
  boxpc_loss dout / terms / loss             2.235e-08 / 1.907e-06 / 0  (2.155e-06 / 1.810e-04 / 2.871e-05)  0.011 / 0.196 / 0.000
  boxpc_loss kink (the seven entry sets)     3.739e-09  (3.313e-07)  0.279   angle dout[:, 6], B=32, switches 10010
  box2d_feats                                0          every ratio the correctly rounded fp32 quotient: no 1-ulp allowance was needed
  act_dropout                                4.768e-07  (5.208e-06)  0.116   M=384 K=67 raw keep0.7 f32; the grid-stride case 4.768e-07, 0.109
  pool_bwd_mid grad / S                      2.861e-06 / 3.338e-06  (1.630e-04 / 1.079e-04)  0.085 / 0.051   byte for byte the two launches
"""
import ctypes as C

import numpy as np
import pytest
import torch

from fake_t3d import MEAN32
from ref_boxpc_b import FakeLibB
from transferable3d_amd import abi
from transferable3d_amd.abi import fptr, iptr
from test_kernels_gpu import _mk, _pool_case

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_SHAPE = -1, -2
GPU = 'cuda'


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    torch.cuda.synchronize()


def _run_both(hip_lib, make, name):
    """make(dev) -> (args, outputs dict).  Runs the spec on CPU and the HIP kernel on the GPU (test_kernels_gpu._run_both with the
    specification library that also has t3d_boxpc_rep_b)."""
    a_c, out_c = make(torch.device('cpu'))
    assert getattr(FakeLibB(), name)(C.byref(a_c), None) == 0
    a_g, out_g = make(torch.device(GPU))
    rc = getattr(hip_lib, name)(C.byref(a_g), _stream())
    assert rc == 0, rc
    _sync()
    return out_c, {k: v.cpu() for k, v in out_g.items()}


def _num(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def _within(what, got, ref, bound):
    """|got - ref| <= bound elementwise; prints the worst error, the bound at that element and the largest share of its bound any
    element used."""
    got, ref = _num(got), _num(ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    used = float(np.max(err / np.maximum(bound, 1e-300)))
    print('%-58s worst %.3e  bound there %.3e  largest error / bound %.3f' % (what, err[i], bound[i], used))
    assert (err <= bound).all(), (what, float(err[i]), float(bound[i]), used, int((err > bound).sum()))


def _close(what, got, ref, rtol, atol):
    _within(what, got, ref, atol + rtol * np.abs(_num(ref)))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(what, a, b):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _fit_logits(r, B):
    """out9[:, 7:9]: ordinary normals; exact ties (p = 0.5); gaps of +-20 and +-100, where the soft-max saturates."""
    lg = r.normal(size=(B, 2)).astype(np.float32)
    lg[1::9, 1] = lg[1::9, 0]
    for k, gap in enumerate((20.0, -20.0, 100.0, -100.0)):
        rows = slice(2 + k, None, 9)
        lg[rows, 0] = np.float32(0.25 * (k - 1))
        lg[rows, 1] = lg[rows, 0] + np.float32(gap)
    return lg


# ---- 1. t3d_box_refine_step_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [37, 300])
@pytest.mark.parametrize('weigh', [0, 1, 2])
@pytest.mark.parametrize('via_conf', [0, 1])
@pytest.mark.parametrize('with_carry', [False, True])
def test_box_refine_step_bwd(hip_lib, B, weigh, via_conf, with_carry):
    """B = 37 (part of one 256-thread block) and 300 (two blocks).

    tot_out = dbox_rep + carry, one fp32 add: rtol 1e-6.
    dout9[:, :7] = -w tot with w = (1 - p)^n, 1 - p formed in fp32 (module docstring): 1e-5 |w tot| + 2^-22 |tot|.
    dout9[:, 7:9] = -+ dot (dw/dp) p q with dot = -sum_k tot_k o_k: the seven products and six adds of dot each round at half an ulp
    of a partial sum that is at most S = sum_k |tot_k o_k|, so |error of dot| <= 13 * 2^-24 S, and |dw/dp p q| <= 0.3 (n = 1: p q <=
    1/4; n = 2: 2 p q^2 <= 8/27): 13 * 0.3 * 2^-24 S < 2^-22 S.  The error of the factor itself (p and q good to a few 2^-24 absolute)
    times |dot| <= S stays below 2^-21 S.  Bound: 1e-5 |value| + 2^-20 S.  Columns 7 and 8 are each other's negation bit for bit."""
    r = np.random.RandomState(100 * B + 10 * weigh + via_conf)
    out9 = r.normal(size=(B, 9)).astype(np.float32)
    out9[:, 7:9] = _fit_logits(r, B)
    d = dict(out9=out9, dbox=r.normal(size=(B, 7)).astype(np.float32), carry=r.normal(size=(B, 7)).astype(np.float32))

    def make(dev):
        t = {k: _mk(dev, v) for k, v in d.items()}
        o = dict(tot=torch.full((B, 7), 7.0, device=dev), dout9=torch.full((B, 9), 7.0, device=dev))
        a = abi.BoxRefineStepBwdArgs(fptr(t['out9']), fptr(t['dbox']), fptr(t['carry'] if with_carry else None), fptr(o['tot']),
                                     fptr(o['dout9']), weigh, via_conf, B)
        a._keep = (t, o)
        return a, o

    c, g = _run_both(hip_lib, make, 't3d_box_refine_step_bwd')
    tag = 'refine_step_bwd B=%d n=%d via=%d carry=%d ' % (B, weigh, via_conf, with_carry)
    _close(tag + 'tot_out', g['tot'], c['tot'], 1e-6, 0.0)
    tot = _num(c['tot'])
    ref = _num(c['dout9'])
    _within(tag + 'dout9[:, :7]', g['dout9'][:, :7], c['dout9'][:, :7], 1e-5 * np.abs(ref[:, :7]) + 2.0 ** -22 * np.abs(tot))
    S = np.abs(tot * out9[:, :7].astype(np.float64)).sum(1, keepdims=True)
    _within(tag + 'dout9[:, 7:9]', g['dout9'][:, 7:9], c['dout9'][:, 7:9], 1e-5 * np.abs(ref[:, 7:9]) + 2.0 ** -20 * S)
    _same_bits(tag + 'dout9[:, 7] == -dout9[:, 8]', g['dout9'][:, 7], -g['dout9'][:, 8])
    if via_conf and weigh:
        assert float(g['dout9'][:, 7].abs().max()) > 0
    else:
        assert float(g['dout9'][:, 7:9].abs().max()) == 0


@pytest.mark.parametrize('B', [37, 300])
@pytest.mark.parametrize('with_carry', [False, True])
def test_box_refine_step_bwd_without_out9_writes_only_tot_out(hip_lib, B, with_carry):
    r = np.random.RandomState(B)
    d = dict(dbox=r.normal(size=(B, 7)).astype(np.float32), carry=r.normal(size=(B, 7)).astype(np.float32))

    def make(dev):
        t = {k: _mk(dev, v) for k, v in d.items()}
        o = dict(tot=torch.full((B, 7), 7.0, device=dev), dout9=torch.full((B, 9), -3.5, device=dev))
        a = abi.BoxRefineStepBwdArgs(None, fptr(t['dbox']), fptr(t['carry'] if with_carry else None), fptr(o['tot']), fptr(o['dout9']),
                                     2, 1, B)
        a._keep = (t, o)
        return a, o

    c, g = _run_both(hip_lib, make, 't3d_box_refine_step_bwd')
    _close('refine_step_bwd out9=NULL B=%d carry=%d tot_out' % (B, with_carry), g['tot'], c['tot'], 1e-6, 0.0)
    assert bool((g['dout9'] == -3.5).all())
    # in place (tot_out = dbox_rep, as the stage-c backward calls it for the unrefined box) and with dout9 = NULL too
    want = torch.as_tensor(d['dbox'] + d['carry'])
    t = {k: _mk(torch.device(GPU), v) for k, v in d.items()}
    a = abi.BoxRefineStepBwdArgs(None, fptr(t['dbox']), fptr(t['carry']), fptr(t['dbox']), None, 0, 0, B)
    assert hip_lib.t3d_box_refine_step_bwd(C.byref(a), _stream()) == 0
    _sync()
    _close('refine_step_bwd out9=NULL in place', t['dbox'], want, 1e-6, 0.0)


# ---- 2. t3d_box_refine_step: the branches test_kernels_gpu.test_box_refine_step leaves out -----------------------------------------------
@pytest.mark.parametrize('weigh,first,with_fit', [(2, 0, True), (1, 1, True), (2, 1, False), (1, 0, False), (0, 0, False)])
def test_box_refine_step_branches(hip_lib, weigh, first, with_fit):
    """test_box_refine_step's 1e-5 / 1e-6, plus 2^-22 |out9_k| on everything that holds w out9_k: w = (1 - p)^n is good to a few
    2^-24 ABSOLUTE only (module docstring)."""
    r = np.random.RandomState(7 + 3 * weigh + first)
    B = 37
    out9 = r.normal(size=(B, 9)).astype(np.float32)
    out9[:, 7:9] = _fit_logits(r, B)
    d = dict(out9=out9, c=r.normal(size=(B, 3)).astype(np.float32), s=(1 + r.uniform(size=(B, 3))).astype(np.float32),
             th=r.normal(size=B).astype(np.float32), tot=r.normal(size=(B, 7)).astype(np.float32))

    def make(dev):
        t = {k: _mk(dev, v) for k, v in d.items()}
        o = dict(c=torch.zeros(B, 3, device=dev), s=torch.zeros(B, 3, device=dev), th=torch.zeros(B, device=dev), tot=t['tot'].clone(),
                 fit=torch.full((B,), -3.5, device=dev))
        a = abi.BoxRefineStepArgs(fptr(t['out9']), fptr(t['c']), fptr(t['s']), fptr(t['th']), fptr(o['c']), fptr(o['s']), fptr(o['th']),
                                  fptr(o['tot']), fptr(o['fit'] if with_fit else None), weigh, first, B)
        a._keep = (t, o)
        return a, o

    c, g = _run_both(hip_lib, make, 't3d_box_refine_step')
    tag = 'refine_step n=%d first=%d fit=%d ' % (weigh, first, with_fit)
    o = np.abs(out9.astype(np.float64))
    for k, ok in (('c', o[:, 0:3]), ('s', o[:, 3:6]), ('th', o[:, 6]), ('tot', o[:, :7])):
        _within(tag + k, g[k], c[k], 1e-6 + 1e-5 * np.abs(_num(c[k])) + 2.0 ** -22 * ok)
    if with_fit:
        _close(tag + 'fit_prob', g['fit'], c['fit'], 1e-5, 1e-6)
        assert float(g['fit'][1]) == 0.5 and float(g['fit'][4]) == 1.0          # the tie; the gap of +100
    else:
        assert bool((g['fit'] == -3.5).all())


# ---- 3. t3d_boxpc_rep_b -------------------------------------------------------------------------------------------------------------
def _box_inputs(r, B, label_form):
    d = dict(center=r.normal(size=(B, 3)).astype(np.float32),
             dims=(r.normal(size=(B, 3)) * 0.1 + (0 if label_form else 1.0)).astype(np.float32),
             theta=(r.uniform(-0.3, 0.3, size=B) + (0 if label_form else 1.0)).astype(np.float32),
             ydc=r.randint(0, 10, size=B).astype(np.int32), yoc=r.randint(0, 12, size=B).astype(np.int32))
    if label_form:
        d['dims'][0] = -5.0                                       # mean + residual < 1e-5: the fmaxf clamp
        d['dims'][B - 1, 1] = -MEAN32[d['ydc'][B - 1], 1]          # ... and exactly 0 before it
    return d


def _rep_b_args(t, o, label_form, shape, B, rpf, Cc, ld_pc, ld_out):
    box, pts = shape in ('box', 'both'), shape in ('points', 'both')
    return abi.BoxPcRepBArgs(fptr(t['center']), fptr(t['dims']), fptr(t['theta']), iptr(t['ydc'] if label_form else None),
                             iptr(t['yoc'] if label_form else None), fptr(o['box'] if box else None), fptr(t['pc']), ld_pc, Cc,
                             fptr(t['mask'] if pts else None), fptr(o['pc_out'] if pts else None), ld_out, B, rpf)


@pytest.mark.parametrize('B', [3, 300])
@pytest.mark.parametrize('rpf', [256, 1000])
@pytest.mark.parametrize('Cc', [3, 4, 6])
def test_boxpc_rep_b_all_launch_shapes(hip_lib, B, rpf, Cc):
    """Box only (grid over B: two blocks at B = 300), points only and both, in the label form and the plain form.  The masked rows are
    products with 0 / 1: bit for bit the spec's fp32.  box_out: 1e-6 against the spec, and bit for bit what t3d_boxpc_rep writes."""
    r = np.random.RandomState(B + rpf + Cc)
    M, ld_pc, ld_out = B * rpf, Cc + 2, Cc + 3
    pc = r.normal(size=(M, ld_pc)).astype(np.float32)
    mask = (r.uniform(size=M) < 0.4).astype(np.float32)
    for label_form in (0, 1):
        d = dict(_box_inputs(r, B, label_form), pc=pc, mask=mask)
        for shape in ('box', 'points', 'both'):
            def make(dev):
                t = {k: _mk(dev, v) for k, v in d.items()}
                o = dict(box=torch.full((B, 7), 7.0, device=dev), pc_out=torch.full((M, ld_out), 7.0, device=dev))
                a = _rep_b_args(t, o, label_form, shape, B, rpf, Cc, ld_pc, ld_out)
                a._keep = (t, o)
                return a, o
            c, g = _run_both(hip_lib, make, 't3d_boxpc_rep_b')
            tag = 'rep_b B=%d rpf=%d C=%d label=%d %s ' % (B, rpf, Cc, label_form, shape)
            if shape == 'box':
                assert bool((g['pc_out'] == 7.0).all())
            else:
                _same_bits(tag + 'pc_out', g['pc_out'], c['pc_out'])
                assert bool((g['pc_out'][:, Cc:] == 0).all())                  # the pad columns
                assert torch.equal(g['pc_out'][:, :Cc], torch.as_tensor(pc[:, :Cc] * mask[:, None]))
            if shape == 'points':
                assert bool((g['box'] == 7.0).all())
                continue
            _close(tag + 'box_out', g['box'], c['box'], 1e-6, 1e-6)
            if label_form:
                assert float(g['box'][0, 3:6].max()) == np.float32(1e-5) and float(g['box'][B - 1, 4]) == np.float32(1e-5)
            # "the arithmetic of load_box": t3d_boxpc_rep's box_out for the same box (it needs rows_per_frustum % 256 == 0)
            dev = torch.device(GPU)
            t = {k: _mk(dev, v) for k, v in d.items() if k not in ('pc', 'mask')}
            pc256, rep, box = torch.zeros(B * 256, 4, device=dev), torch.zeros(B * 256, 10, device=dev), torch.full((B, 7), 7.0, device=dev)
            a = abi.BoxPcRepArgs(fptr(pc256), 4, 4, fptr(t['center']), fptr(t['dims']), fptr(t['theta']),
                                 iptr(t['ydc'] if label_form else None), iptr(t['yoc'] if label_form else None), fptr(rep), 10, fptr(box),
                                 B * 256, 256, None)
            assert hip_lib.t3d_boxpc_rep(C.byref(a), _stream()) == 0
            _sync()
            _same_bits(tag + 'box_out == t3d_boxpc_rep box_out', g['box'], box.cpu())


def test_boxpc_rep_b_refuses_bad_arguments(hip_lib):
    dev = torch.device(GPU)
    B, rpf, Cc = 3, 256, 4
    r = np.random.RandomState(1)
    t = {k: _mk(dev, v) for k, v in _box_inputs(r, B, 1).items()}
    t['pc'], t['mask'] = torch.zeros(B * rpf, Cc, device=dev), torch.ones(B * rpf, device=dev)
    o = dict(box=torch.zeros(B, 7, device=dev), pc_out=torch.zeros(B * rpf, Cc, device=dev))
    call = lambda a: hip_lib.t3d_boxpc_rep_b(C.byref(a), _stream())
    a = _rep_b_args(t, o, 1, 'both', B, rpf, Cc, Cc, Cc)
    assert call(a) == 0
    a = _rep_b_args(t, o, 1, 'both', B, rpf, Cc, Cc, Cc)
    a.box_out, a.pc_out = None, None                                     # both outputs NULL
    assert call(a) == ERR_ARG
    a.rowmask = None
    assert call(a) == ERR_ARG
    assert call(_rep_b_args(t, o, 1, 'both', B, rpf, Cc, Cc, Cc - 1)) == ERR_SHAPE          # ld_out < C
    assert call(_rep_b_args(t, o, 1, 'points', B, rpf, Cc, Cc, Cc - 1)) == ERR_SHAPE
    a = _rep_b_args(t, o, 1, 'box', B, rpf, Cc, Cc, Cc)
    a.y_orient_cls = None                                                # y_dims_cls without y_orient_cls
    assert call(a) == ERR_ARG
    _sync()


# ---- 4. t3d_boxpc_rep with rowmask (--mask_pc_for_boxpc) ---------------------------------------------------------------------------------
@pytest.mark.parametrize('Cc', [4, 6])
@pytest.mark.parametrize('label_form', [0, 1])
def test_boxpc_rep_with_rowmask(hip_lib, Cc, label_form):
    r = np.random.RandomState(50 + Cc)
    B, rpf = 5, 256
    M, ld_pc, ld = B * rpf, Cc + 1, Cc + 6 + 3
    pc = r.normal(size=(M, ld_pc)).astype(np.float32)
    mask = (r.uniform(size=M) < 0.4).astype(np.float32)
    mask[:rpf] = 0                                                      # one frustum fully masked,
    mask[rpf:2 * rpf] = 1                                               # one fully kept
    d = dict(_box_inputs(r, B, label_form), pc=pc, mask=mask)

    def make(dev):
        t = {k: _mk(dev, v) for k, v in d.items()}
        o = dict(rep=torch.full((M, ld), 7.0, device=dev), box=torch.zeros(B, 7, device=dev))
        a = abi.BoxPcRepArgs(fptr(t['pc']), ld_pc, Cc, fptr(t['center']), fptr(t['dims']), fptr(t['theta']),
                             iptr(t['ydc'] if label_form else None), iptr(t['yoc'] if label_form else None), fptr(o['rep']), ld,
                             fptr(o['box']), M, rpf, fptr(t['mask']))
        a._keep = (t, o)
        return a, o

    c, g = _run_both(hip_lib, make, 't3d_boxpc_rep')
    tag = 'rep rowmask C=%d label=%d ' % (Cc, label_form)
    _close(tag + 'rep', g['rep'], c['rep'], 1e-5, 1e-5)
    _close(tag + 'box', g['box'], c['box'], 1e-6, 1e-6)
    assert bool((g['rep'][:, Cc + 6:] == 0).all())                         # the pad columns
    assert bool((g['rep'][:rpf, :Cc] == 0).all()) and torch.equal(g['rep'][rpf:2 * rpf, :Cc], torch.as_tensor(pc[rpf:2 * rpf, :Cc]))

    def make_b(dev):
        t = {k: _mk(dev, v) for k, v in d.items()}
        o = dict(box=torch.zeros(B, 7, device=dev), pc_out=torch.full((M, Cc + 2), 7.0, device=dev))
        a = _rep_b_args(t, o, label_form, 'both', B, rpf, Cc, ld_pc, Cc + 2)
        a._keep = (t, o)
        return a, o
    _, gb = _run_both(hip_lib, make_b, 't3d_boxpc_rep_b')
    _same_bits(tag + 'rep[:, :C] == rep_b pc_out', g['rep'][:, :Cc].contiguous(), gb['pc_out'][:, :Cc].contiguous())
    _same_bits(tag + 'box == rep_b box_out', g['box'], gb['box'])


# ---- 5. t3d_boxpc_rep_bwd: the 256-stride loop below one pass, at one pass, with a ragged last pass ----------------------------------------
@pytest.mark.parametrize('rpf', [100, 256, 1000])
@pytest.mark.parametrize('Cc,coff', [(3, 2), (6, 8)])
def test_boxpc_rep_bwd_shapes(hip_lib, rpf, Cc, coff):
    r = np.random.RandomState(rpf + Cc)
    B = 5
    M, ld_pc, ld_drep = B * rpf, Cc + 1, coff + 6 + 3
    d = dict(pc=r.normal(size=(M, ld_pc)).astype(np.float32), drep=(r.normal(size=(M, ld_drep)) * 1e-2).astype(np.float32),
             box=np.concatenate([r.normal(size=(B, 3)), 1 + r.uniform(size=(B, 3)), r.uniform(-3, 3, size=(B, 1))], 1).astype(np.float32))

    def make(dev):
        t = {k: _mk(dev, v) for k, v in d.items()}
        o = dict(dbox=torch.full((B, 7), 7.0, device=dev))
        a = abi.BoxPcRepBwdArgs(fptr(t['pc']), ld_pc, fptr(t['box']), fptr(t['drep']), ld_drep, coff, fptr(o['dbox']), B, rpf)
        a._keep = (t, o)
        return a, o

    c, g = _run_both(hip_lib, make, 't3d_boxpc_rep_bwd')
    _close('rep_bwd rpf=%d C=%d coff=%d dbox' % (rpf, Cc, coff), g['dbox'], c['dbox'], 1e-4, 1e-5)


# ---- 6. t3d_boxpc_loss: weigh_pred_by_cls_conf, grad_cls_via_delta, delta_loss_mse ------------------------------------------------------
# (weigh_by_cls_conf, weigh_by_cls_gt, weigh_pred_by_cls_conf, grad_cls_via_delta, delta_loss_mse): each new switch alone, then what
# test_off_recipe_cpu.BOXPC_VARIANTS sets (nets.BoxPcLoss.emit maps the flags; tests/test_glue_spec_cpu.py holds the list against them)
LOSS_SWITCHES = [(0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (0, 0, 1, 1, 0), (1, 0, 0, 1, 0), (1, 0, 1, 1, 1), (0, 1, 1, 1, 0)]


@pytest.mark.parametrize('B', [32, 1000])               # t3d_boxpc_loss takes B <= 1024: one 1024-thread workgroup, nearly full at 1000
@pytest.mark.parametrize('sw', LOSS_SWITCHES, ids=lambda s: ''.join(map(str, s)))
def test_boxpc_loss_switches(hip_lib, B, sw):
    r = np.random.RandomState(B + int(''.join(map(str, sw)), 2))
    out9 = r.normal(size=(B, 9)).astype(np.float32)
    iou = r.uniform(size=B).astype(np.float32)
    iou[::5] = np.float32(0.7)                                           # exactly at fit_bound: not above it
    dc, ds, da = [(r.normal(size=s) * 0.7).astype(np.float32) for s in ((B, 3), (B, 3), (B,))]
    # the Huber kink: targets of exactly +-1 against a prediction of 0, and an error of exactly +-1 from exact halves
    dc[1::4], ds[2::4, 1], da[3::4] = 1.0, -1.0, -1.0
    out9[1::4, 0:3], out9[2::4, 4], out9[3::4, 6] = 0.0, 0.0, 0.0
    out9[0::8, 3], ds[0::8, 0] = 0.5, -0.5
    out9[4::8, 6], da[4::8] = -0.5, 0.5
    conf, gt, pred, via, mse = sw

    def make(dev):
        t = {k: _mk(dev, v) for k, v in dict(o=out9, iou=iou, dc=dc, ds=ds, da=da).items()}
        o = dict(dout=torch.full((B, 9), 7.0, device=dev), terms=torch.full((B, 4), 7.0, device=dev), loss=torch.zeros(1, device=dev))
        a = abi.BoxPcLossArgs(fptr(t['o']), fptr(t['iou']), fptr(t['dc']), fptr(t['ds']), fptr(t['da']), 0.7, 1.0, 4.0, 0.34, 0.33, 0.33,
                              conf, gt, fptr(o['dout']), fptr(o['terms']), fptr(o['loss']), B, pred, via, mse)
        a._keep = (t, o)
        return a, o

    c, g = _run_both(hip_lib, make, 't3d_boxpc_loss')
    for k in c:
        _close('boxpc_loss B=%d %s %s' % (B, ''.join(map(str, sw)), k), g[k], c[k], 1e-5, 1e-6)
    if pred or mse:
        return
    # The Huber kink.  With wp = 1 and the Huber form every entry set up above has an error of exactly +-1, where the quadratic and the
    # linear branch meet and the clamp convention gives a derivative of exactly +-1: dout = sign w_delta wl w_k / (3 B) (w_angle: / B), wl
    # = 1, 1 - iou or 1 - p_fit.  The coefficient is a handful of fp32 products (1e-5 relative); wl = 1 - p_fit is formed in fp32 and
    # carries a few 2^-24 absolute (module docstring): 2^-22 of the coefficient.
    lg = out9[:, 7:9].astype(np.float64)
    p_fit = 1.0 / (1.0 + np.exp(lg[:, 0] - lg[:, 1]))
    wl = 1.0 - p_fit if conf else 1.0 - iou.astype(np.float64) if gt else np.ones(B)
    got = _num(g['dout'])
    for what, rows, col, sign, wk in (('center', slice(1, None, 4), 0, -1, 0.34 / 3), ('center', slice(1, None, 4), 1, -1, 0.34 / 3),
                                      ('center', slice(1, None, 4), 2, -1, 0.34 / 3), ('size', slice(2, None, 4), 4, 1, 0.33 / 3),
                                      ('angle', slice(3, None, 4), 6, 1, 0.33), ('size from halves', slice(0, None, 8), 3, 1, 0.33 / 3),
                                      ('angle from halves', slice(4, None, 8), 6, -1, 0.33)):
        coef = 4.0 * wk / B
        want = sign * coef * wl[rows]
        _within('boxpc_loss B=%d %s kink %s dout[:, %d]' % (B, ''.join(map(str, sw)), what, col), got[rows, col], want,
                1e-5 * np.abs(want) + 2.0 ** -22 * coef)


def test_boxpc_loss_refuses_more_than_one_workgroup(hip_lib):
    z = torch.zeros(1025 * 9, device=GPU)
    a = abi.BoxPcLossArgs(fptr(z), fptr(z), fptr(z), fptr(z), fptr(z), 0.7, 1.0, 4.0, 0.34, 0.33, 0.33, 0, 0, fptr(z), fptr(z), fptr(z),
                          1025, 0, 0, 0)
    assert hip_lib.t3d_boxpc_loss(C.byref(a), _stream()) == ERR_SHAPE


# ---- 7. t3d_box2d_feats -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_oh', [0, 10])
def test_box2d_feats(hip_lib, n_oh):
    """Non-square images (rows != cols: a swap of the two shows), boxes in pixels.  The one-hot columns are a copy; each ratio is one
    fp32 division, and the library is built without fast-math, so it is the correctly rounded np.float32(a) / np.float32(b)."""
    r = np.random.RandomState(70 + n_oh)
    B = 37
    dim = np.tile(np.array([[530.0, 730.0]], np.float32), (B, 1))          # (rows, cols)
    dim[1::3] = (427.0, 561.0)
    dim[2::3] = (730.0, 530.0)
    rows, cols = dim[:, 0], dim[:, 1]
    box = np.stack([r.uniform(0, 0.5, B) * cols, r.uniform(0, 0.5, B) * rows, r.uniform(0.5, 1, B) * cols, r.uniform(0.5, 1, B) * rows],
                   1).astype(np.float32)
    oh = r.normal(size=(B, max(n_oh, 1))).astype(np.float32)               # (any values: they are copied)

    def make(dev):
        t = {k: _mk(dev, v) for k, v in dict(oh=oh, box=box, dim=dim).items()}
        o = dict(out=torch.full((B, n_oh + 4), 7.0, device=dev))
        a = abi.Box2dFeatsArgs(fptr(t['oh'] if n_oh else None), n_oh, fptr(t['box']), fptr(t['dim']), fptr(o['out']), B)
        a._keep = (t, o)
        return a, o

    c, g = _run_both(hip_lib, make, 't3d_box2d_feats')
    _same_bits('box2d_feats n_oh=%d spec' % n_oh, g['out'], c['out'])
    want = np.stack([box[:, 0] / cols, box[:, 1] / rows, box[:, 2] / cols, box[:, 3] / rows], 1)
    assert want.dtype == np.float32
    _same_bits('box2d_feats ratios', g['out'][:, n_oh:].contiguous(), torch.as_tensor(want))
    if n_oh:
        _same_bits('box2d_feats one-hot copy', g['out'][:, :n_oh].contiguous(), torch.as_tensor(oh))
    print('%-58s worst %.3e  bound there %.3e' % ('box2d_feats n_oh=%d (correctly rounded division)' % n_oh, 0.0, 0.0))


def test_box2d_feats_refuses_a_missing_one_hot(hip_lib):
    z = torch.ones(37 * 14, device=GPU)
    a = abi.Box2dFeatsArgs(None, 10, fptr(z), fptr(z), fptr(z), 37)
    assert hip_lib.t3d_box2d_feats(C.byref(a), _stream()) == ERR_ARG


# ---- 8. t3d_act_dropout ---------------------------------------------------------------------------------------------------------------
def _act_dropout_case(hip_lib, M, K, rpf, form, mask_form, dtype, seed):
    """out = act(a) * mask / keep: one fma, one max, one subtract, two multiplies (1 / keep is a third rounding), each half an ulp of
    a result that only grows in magnitude along the chain of one source form: 1e-6 relative + 1e-7 absolute."""
    r = np.random.RandomState(seed)
    B = M // rpf
    coff, ldx = (5, 5 + K + 3) if form == 'coff' else (0, K)
    x = torch.as_tensor(r.normal(size=(M, ldx)).astype(np.float32))
    if dtype == abi.BF16:
        x = x.bfloat16()
    sc = (0.5 + r.uniform(size=K)).astype(np.float32)
    sc[::3] *= -1
    d = dict(sc=sc, sh=(r.normal(size=K) * 0.2).astype(np.float32), sub=r.normal(size=(B, K + 5)).astype(np.float32),
             mask=(r.uniform(size=(M, K)) < 0.7).astype(np.float32))
    keep = {'none': 0.7, 'keep0.7': 0.7, 'keep1.0': 1.0}[mask_form]

    def make(dev):
        t = {k: _mk(dev, v) for k, v in d.items()}
        # the spec reads an fp32 source (fake_t3d._act): the bf16 one is widened on the host for it, exactly
        t['x'] = x.to(dev) if dev.type != 'cpu' else x.float()
        o = dict(out=torch.full((M, K), 7.0, device=dev))
        src = abi.ActSrc(fptr(t['x']), ldx, coff, fptr(t['sc'] if form == 'bn_relu' else None), fptr(t['sh'] if form == 'bn_relu' else None),
                         int(form == 'bn_relu'), fptr(t['sub'] if form == 'sub' else None), K + 5,
                         dtype if dev.type != 'cpu' else abi.F32)
        a = abi.ActDropoutArgs(src, fptr(None if mask_form == 'none' else t['mask']), keep, fptr(o['out']), M, K, rpf)
        a._keep = (t, o)
        return a, o

    c, g = _run_both(hip_lib, make, 't3d_act_dropout')
    _close('act_dropout M=%d K=%d %s %s %s' % (M, K, form, mask_form, 'bf16' if dtype else 'f32'), g['out'], c['out'], 1e-6, 1e-7)
    if mask_form != 'none':
        assert bool((g['out'][torch.as_tensor(d['mask']) == 0] == 0).all())
    return g['out']


@pytest.mark.parametrize('form', ['raw', 'bn_relu', 'sub', 'coff'])
@pytest.mark.parametrize('mask_form', ['none', 'keep0.7', 'keep1.0'])
@pytest.mark.parametrize('dtype', [abi.F32, abi.BF16], ids=['f32', 'bf16'])
def test_act_dropout(hip_lib, form, mask_form, dtype):
    _act_dropout_case(hip_lib, 384, 67, 128, form, mask_form, dtype, 80)


def test_act_dropout_grid_stride_tail(hip_lib):
    """4096 x 520 = 2,129,920 elements against the launch's cap of 8192 x 256 = 2,097,152 threads: the last 32,768 elements are reached
    only through the grid-stride loop."""
    out = _act_dropout_case(hip_lib, 4096, 520, 1024, 'raw', 'keep0.7', abi.F32, 81)
    assert float(out.reshape(-1)[8192 * 256:].abs().max()) > 0


# ---- 9. t3d_pool_bwd_mid ----------------------------------------------------------------------------------------------------------------
SENTINEL = -3.5


@pytest.mark.parametrize('M,K,N,rpf', [(512, 128, 1024, 256), (256, 256, 512, 128)])
def test_pool_bwd_mid_equals_reduce_slabs_then_sparse_rows(hip_lib, M, K, N, rpf):
    """One launch against t3d_reduce_slabs followed by t3d_pool_sparse_rows from identical inputs: byte for byte (both run the same
    bodies), the spec at the tolerances of test_reduce_slabs_adam_schedule_dropout and test_pool_sparse_rows, and a sentinel around every
    output untouched (a wrong split between the two kinds of workgroup writes, or leaves out, a neighbouring tile)."""
    r = np.random.RandomState(M + N)
    # (n_slabs, numel): 70 slabs take every unrolling of the float4 path; 36992 / 4 elements are more than the 256 x 32 one pass of the
    # widest grid covers; 67 is no multiple of 4 (t3d_reduce_slabs takes it: the scalar path)
    sizes = [(70, 640), (9, 36992), (3, 67)]
    slab = np.concatenate([r.normal(size=ns * ne) for ns, ne in sizes]).astype(np.float32)
    table = (abi.SlabDesc * 3)()
    so, go = 0, 8
    for i, (ns, ne) in enumerate(sizes):
        table[i] = abi.SlabDesc(so, go, ne, ns)
        so += ns * ne
        go += ne + 4
    max_numel = max(ne for _, ne in sizes)
    d = _pool_case(M, K, N, rpf, M + K)
    wc = np.ascontiguousarray((d['w'] * d['coef'][0]).T)
    pad = 256

    def buffers(dev):
        t = {k: _mk(dev, v) for k, v in dict(argidx=d['argidx'], dpool=d['dpool'], wc=wc, slab=slab).items()}
        t['grad'] = torch.full((go + pad,), SENTINEL, device=dev)
        t['s'] = torch.full((pad + M * K + pad,), SENTINEL, device=dev)
        s = t['s'][pad:pad + M * K]
        assert s.data_ptr() % 16 == 0
        t['sparse'] = abi.PoolSparseRowsArgs(iptr(t['argidx']), fptr(t['dpool']), fptr(t['wc']), M // rpf, N, K, rpf, fptr(s), None)
        return t

    spec = buffers(torch.device('cpu'))
    assert FakeLibB().t3d_pool_bwd_mid(fptr(spec['slab']), fptr(spec['grad']), table, 3, max_numel, C.byref(spec['sparse']), None) == 0
    dev = torch.device(GPU)
    tab_dev = torch.as_tensor(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
    tab = C.cast(C.c_void_p(tab_dev.data_ptr()), C.POINTER(abi.SlabDesc))
    apart, fused = buffers(dev), buffers(dev)
    assert hip_lib.t3d_reduce_slabs(fptr(apart['slab']), fptr(apart['grad']), tab, 3, max_numel, _stream()) == 0
    assert hip_lib.t3d_pool_sparse_rows(C.byref(apart['sparse']), _stream()) == 0
    assert hip_lib.t3d_pool_bwd_mid(fptr(fused['slab']), fptr(fused['grad']), tab, 3, max_numel, C.byref(fused['sparse']), _stream()) == 0
    _sync()
    tag = 'pool_bwd_mid M=%d K=%d N=%d ' % (M, K, N)
    for k in ('grad', 's'):
        _same_bits(tag + k + ': fused == separate', fused[k], apart[k])
    # the sentinels: in front of, between and behind the gradient regions; around S
    live = torch.zeros(go + pad, dtype=torch.bool)
    for i in range(3):
        live[table[i].grad_off:table[i].grad_off + table[i].numel] = True
    grad = fused['grad'].cpu()
    assert bool((grad[~live] == SENTINEL).all()) and bool((spec['grad'][~live] == SENTINEL).all())
    s = fused['s'].cpu()
    assert bool((s[:pad] == SENTINEL).all()) and bool((s[pad + M * K:] == SENTINEL).all())
    _close(tag + 'grad', grad[live], spec['grad'][live], 1e-5, 1e-5)
    s_ref = spec['s'][pad:pad + M * K]
    _close(tag + 'S', s[pad:pad + M * K], s_ref, 1e-5, 1e-5 * float(s_ref.abs().max()))
    assert float(s_ref.abs().max()) > 0
