"""CPU: the NumPy specifications of the refinement step's backward, of the Box-PC representation's backward and of the 2-D box
features (tests/fake_t3d.py) checked against something that was NOT written alongside the kernels -- a central finite difference of
the matching forward specification, the oracle's restatement of the reference -- so that tests/test_kernels_glue_gpu.py compares the
HIP kernels with specifications that stand on their own.  Also: no training graph hands a row mask to the Box-PC representation,
whose backward kernel has none; and the switch sets the GPU module gives t3d_boxpc_loss include those of the off-recipe variants.

Finite differences: the specification library writes fp32 buffers, and an fp32 rounding (6e-8) divided by a step of 1e-4 would swamp
the comparison, so each forward is restated here in fp64 in the specification's own few lines and that restatement is first held
against the specification's fp32 output (to fp32 rounding).  With h = 1e-4 on O(1) inputs the central difference of these smooth
functions is off by h^2 f''' / 6 ~ 2e-9 and by eps / h ~ 1e-12 of rounding; the specification's gradient comes back through an fp32
buffer (6e-8 relative).  Agreement is asked to 1e-6 of the largest gradient entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from fake_t3d import FakeLib
from transferable3d_amd import abi
from transferable3d_amd.abi import fptr

H = 1e-4
AGREE = 1e-6


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))


def _central_difference(f, x):
    """d f / d x[i] of a scalar f at the fp64 array x, entry by entry."""
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += H
        xm[i] -= H
        g[i] = (f(xp) - f(xm)) / (2 * H)
    return g


# ---- refinement step -------------------------------------------------------------------------------------------------------------------
def _refine_forward64(out9, box, n):
    """FakeLib.t3d_box_refine_step in fp64: [center_out | dims_out | theta_out] = box - (1 - p_fit)^n out9[:, :7]."""
    z = out9[:, 7:9] - out9[:, 7:9].max(1, keepdims=True)
    pfit = np.exp(z[:, 1]) / np.exp(z).sum(1)
    w = (1.0 - pfit) ** n
    return box - out9[:, :7] * w[:, None]


def _refine_case(seed, B=6):
    r = np.random.RandomState(seed)
    out9 = r.normal(size=(B, 9)).astype(np.float32)
    out9[1, 8] = out9[1, 7]                                               # a tie
    box = np.concatenate([r.normal(size=(B, 3)), 1 + r.uniform(size=(B, 3)), r.normal(size=(B, 1))], 1).astype(np.float32)
    g = r.normal(size=(B, 7)).astype(np.float32)
    return out9, box, g


def _spec_refine_bwd(out9, g, n, via_conf, split_carry):
    """dout9 of FakeLib.t3d_box_refine_step_bwd for L = sum g * [center_out | dims_out | theta_out].

    Sign convention, from the caller (nets.SemiModelF.emit_backward): `dbox_rep` and `carry` are PLAIN gradients dL/d(box_i) -- what
    t3d_boxpc_rep_bwd / the box MLP's input gradient and the step behind deliver, no sign applied -- and the entry point itself applies
    the minus sign of box_i = box_{i-1} - w delta_{i-1}: dout9[:, :7] = -w tot.  So dL/d(box_out) = g goes in as it is (split over
    dbox_rep and carry, whose sum is all that matters), and dout9 must come out as dL/d(out9)."""
    B = out9.shape[0]
    carry = 0.25 * g if split_carry else None
    t = dict(out9=_t(out9), dbox=_t(g - carry if split_carry else g), carry=_t(carry) if split_carry else None)
    o = dict(tot=torch.zeros(B, 7), dout9=torch.full((B, 9), 7.0))
    a = abi.BoxRefineStepBwdArgs(fptr(t['out9']), fptr(t['dbox']), fptr(t['carry']), fptr(o['tot']), fptr(o['dout9']), n, via_conf, B)
    assert FakeLib().t3d_box_refine_step_bwd(C.byref(a), None) == 0
    return o['dout9'].double().numpy(), o['tot'].double().numpy()


@pytest.mark.parametrize('n', [0, 1, 2])
def test_refine_forward_restatement_is_the_specification(n):
    out9, box, _ = _refine_case(n)
    B = out9.shape[0]
    t = dict(out9=_t(out9), c=_t(box[:, 0:3]), s=_t(box[:, 3:6]), th=_t(box[:, 6]))
    o = dict(c=torch.zeros(B, 3), s=torch.zeros(B, 3), th=torch.zeros(B), tot=torch.zeros(B, 7))
    a = abi.BoxRefineStepArgs(fptr(t['out9']), fptr(t['c']), fptr(t['s']), fptr(t['th']), fptr(o['c']), fptr(o['s']), fptr(o['th']),
                              fptr(o['tot']), None, n, 1, B)
    assert FakeLib().t3d_box_refine_step(C.byref(a), None) == 0
    spec = torch.cat([o['c'], o['s'], o['th'][:, None]], 1).double().numpy()
    mine = _refine_forward64(out9.astype(np.float64), box.astype(np.float64), n)
    assert np.abs(spec - mine).max() <= 2.0 ** -23 * np.abs(mine).max()


@pytest.mark.parametrize('n', [0, 1, 2])
@pytest.mark.parametrize('split_carry', [False, True])
def test_refine_backward_is_the_derivative_of_the_forward(n, split_carry):
    out9, box, g = _refine_case(10 + n)
    o64, b64, g64 = out9.astype(np.float64), box.astype(np.float64), g.astype(np.float64)
    fd = _central_difference(lambda o: float((g64 * _refine_forward64(o, b64, n)).sum()), o64)
    dout9, tot = _spec_refine_bwd(out9, g, n, 1, split_carry)
    scale = np.abs(dout9).max()
    assert np.abs(dout9 - fd).max() <= AGREE * scale, (np.abs(dout9 - fd).max(), scale)
    assert np.abs(tot - g64).max() <= 2.0 ** -23 * np.abs(g64).max()          # d box_out / d box_in = 1: the carry for the step before
    if n:
        assert np.abs(fd[:, 7:9]).max() > 1e-3 * scale                       # (the confidence columns carry a real gradient)
    else:
        assert np.abs(fd[:, 7:9]).max() <= AGREE * scale and np.abs(dout9[:, 7:9]).max() == 0


@pytest.mark.parametrize('n', [1, 2])
def test_refine_backward_with_the_confidence_detached(n):
    """grad_via_conf = 0 (BOXPC_STOP_GRAD_OF_CLS_VIA_DELTA): columns 7 and 8 are 0 although the function does depend on them; the
    delta columns are unchanged."""
    out9, box, g = _refine_case(20 + n)
    o64, b64, g64 = out9.astype(np.float64), box.astype(np.float64), g.astype(np.float64)
    fd = _central_difference(lambda o: float((g64 * _refine_forward64(o, b64, n)).sum()), o64)
    dout9, _ = _spec_refine_bwd(out9, g, n, 0, False)
    scale = np.abs(fd).max()
    assert np.abs(dout9[:, 7:9]).max() == 0 and np.abs(fd[:, 7:9]).max() > 1e-3 * scale
    assert np.abs(dout9[:, :7] - fd[:, :7]).max() <= AGREE * scale


# ---- Box-PC representation -------------------------------------------------------------------------------------------------------------
RPF, CC = 100, 4


def _rep_distances64(pc, box):
    """The six distance columns of FakeLib.t3d_boxpc_rep in fp64, box = [cx, cy, cz, l, w, h, theta] per frustum."""
    B = box.shape[0]
    rep = lambda v: np.repeat(v, RPF)
    t = pc[:, :3] - np.repeat(box[:, 0:3], RPF, 0)
    c, s = rep(np.cos(box[:, 6])), rep(np.sin(box[:, 6]))
    l, w, h = rep(box[:, 3]), rep(box[:, 4]), rep(box[:, 5])
    u, q = c * t[:, 0] - s * t[:, 2], s * t[:, 0] + c * t[:, 2]
    assert pc.shape[0] == B * RPF
    return np.stack([l / 2 - u, l / 2 + u, h / 2 - t[:, 1], h / 2 + t[:, 1], w / 2 - q, w / 2 + q], 1)


def _rep_case(seed, B=3):
    r = np.random.RandomState(seed)
    pc = r.normal(size=(B * RPF, CC)).astype(np.float32)
    box = np.concatenate([r.normal(size=(B, 3)), 1 + r.uniform(size=(B, 3)), r.uniform(-3, 3, size=(B, 1))], 1).astype(np.float32)
    G = r.normal(size=(B * RPF, 6)).astype(np.float32)
    return pc, box, G


def test_rep_forward_restatement_is_the_specification():
    pc, box, _ = _rep_case(1)
    B, M, ld = box.shape[0], pc.shape[0], CC + 6 + 2
    t = dict(pc=_t(pc), c=_t(box[:, 0:3]), s=_t(box[:, 3:6]), th=_t(box[:, 6]))
    o = dict(rep=torch.full((M, ld), 7.0), box=torch.zeros(B, 7))
    a = abi.BoxPcRepArgs(fptr(t['pc']), CC, CC, fptr(t['c']), fptr(t['s']), fptr(t['th']), None, None, fptr(o['rep']), ld, fptr(o['box']),
                         M, RPF, None)
    assert FakeLib().t3d_boxpc_rep(C.byref(a), None) == 0
    assert np.array_equal(o['box'].numpy(), box)                          # the 7-vector the backward reads: [centre | l, w, h | theta]
    mine = _rep_distances64(pc.astype(np.float64), box.astype(np.float64))
    assert np.abs(o['rep'][:, CC:CC + 6].double().numpy() - mine).max() <= 2.0 ** -23 * np.abs(mine).max()


def test_rep_backward_is_the_derivative_of_the_six_distance_columns():
    """L = sum G * rep[:, C:C+6]; dbox of FakeLib.t3d_boxpc_rep_bwd = dL / d[cx, cy, cz, l, w, h, theta], at rows_per_frustum = 100."""
    pc, box, G = _rep_case(2)
    B, M = box.shape[0], pc.shape[0]
    p64, b64, G64 = pc.astype(np.float64), box.astype(np.float64), G.astype(np.float64)
    fd = _central_difference(lambda b: float((G64 * _rep_distances64(p64, b)).sum()), b64)
    coff, ld = 3, 3 + 6 + 2
    drep = np.full((M, ld), 7.0, np.float32)                              # (what lies around the six columns is not read)
    drep[:, coff:coff + 6] = G
    t = dict(pc=_t(pc), box=_t(box), drep=_t(drep))
    dbox = torch.full((B, 7), 7.0)
    a = abi.BoxPcRepBwdArgs(fptr(t['pc']), CC, fptr(t['box']), fptr(t['drep']), ld, coff, fptr(dbox), B, RPF)
    assert FakeLib().t3d_boxpc_rep_bwd(C.byref(a), None) == 0
    got = dbox.double().numpy()
    scale = np.abs(got).max()
    assert np.abs(got - fd).max() <= AGREE * scale, (np.abs(got - fd).max(), scale)
    assert (np.abs(fd) > 1e-3 * scale).all()                               # every one of the 7 entries is exercised


# ---- 2-D box features --------------------------------------------------------------------------------------------------------------------
def test_box2d_feats_spec_is_the_oracles_norm_box2d_on_a_non_square_image():
    """oracle.ref_torch.tf_normalize_2D_bboxes restates the reference (models/tf_util.py:466-484: image_dim = (rows, cols); left and
    right over cols, top and bottom over rows).  The specification divides in fp32: half an ulp."""
    from oracle import ref_torch as R
    r = np.random.RandomState(5)
    B, n_oh = 9, 10
    dim = np.tile(np.array([[530.0, 730.0]], np.float32), (B, 1))
    dim[1::2] = (427.0, 561.0)
    box = (r.uniform(size=(B, 4)) * np.array([730.0, 530.0, 730.0, 530.0])).astype(np.float32)
    oh = np.eye(n_oh, dtype=np.float32)[r.randint(0, n_oh, size=B)]
    t = dict(oh=_t(oh), box=_t(box), dim=_t(dim))
    out = torch.full((B, n_oh + 4), 7.0)
    a = abi.Box2dFeatsArgs(fptr(t['oh']), n_oh, fptr(t['box']), fptr(t['dim']), fptr(out), B)
    assert FakeLib().t3d_box2d_feats(C.byref(a), None) == 0
    ref = R.tf_normalize_2D_bboxes(torch.as_tensor(box, dtype=torch.float64), torch.as_tensor(dim, dtype=torch.float64)).numpy()
    assert np.abs(out[:, n_oh:].double().numpy() - ref).max() <= 2.0 ** -24 * np.abs(ref).max()
    assert np.array_equal(out[:, :n_oh].numpy(), oh)
    swapped = np.stack([box[:, 0] / dim[:, 0], box[:, 1] / dim[:, 1], box[:, 2] / dim[:, 0], box[:, 3] / dim[:, 1]], 1)
    assert np.abs(swapped - ref).max() > 0.01                              # (rows and cols exchanged would show)


# ---- no training graph masks the Box-PC representation's points ---------------------------------------------------------------------
def _rowmasks(plan):
    return [(n, bool(a.rowmask)) for n, _, a in plan.calls if n in ('t3d_boxpc_rep', 't3d_boxpc_rep_b')]


@pytest.mark.parametrize('rep', ['A', 'B'])
def test_no_training_graph_passes_a_rowmask_to_the_boxpc_representation(rep):
    """k_boxpc_rep_bwd reads the unmasked point cloud (it has no rowmask), while t3d_boxpc_rep's forward may see pc * rowmask
    (--mask_pc_for_boxpc).  That is consistent as long as only the inference graph, which has no backward, passes a mask."""
    import test_boxpc_rep_b_cpu as TB
    from transferable3d_amd.nets import Graph, SemiModelF
    from transferable3d_amd.step import build_training_step, workload_flags
    rt = TB._runtime()
    fc = TB._stage_c_flags(3, True)                                       # stage c, the gradient running back through two refinement steps
    fc.BOX_PC_MASK_REPRESENTATION = rep
    g, _ = TB._stage_c_step(rt, fc)
    fb = workload_flags('boxpc')                                          # stage b
    fb.BOX_PC_MASK_REPRESENTATION = rep
    gb = build_training_step(rt, 'boxpc', TB.SHAPE[0], TB.SHAPE[1], TB.C, c=fb, use_hip_graph=False)[0]
    for graph in (g, gb):
        seen = _rowmasks(graph.fwd) + _rowmasks(graph.bwd)
        assert seen and not any(masked for _, masked in seen), seen
    if rep == 'A':
        assert 't3d_boxpc_rep_bwd' in [n for n, _, _ in g.bwd.calls]
    # the inference graph with mask_pc_for_boxpc does pass one (so the assertion above can see a mask), and has no backward
    gi = Graph(TB.SHAPE[0], TB.SHAPE[1], TB.C, rt=rt)
    m = SemiModelF(gi, fc, use_one_hot=True, mask_pc_for_boxpc=True)
    m.refine_num = 2
    m.emit_forward(gi.fwd, False, False)
    assert any(masked for _, masked in _rowmasks(gi.fwd)) and len(gi.bwd) == 0


# ---- the t3d_boxpc_loss switch sets of the GPU module ----------------------------------------------------------------------------------
def test_loss_switches_cover_the_off_recipe_variants():
    """test_kernels_glue_gpu.LOSS_SWITCHES holds every (weigh_by_cls_conf, weigh_by_cls_gt, weigh_pred_by_cls_conf, grad_cls_via_delta,
    delta_loss_mse) that test_off_recipe_cpu.BOXPC_VARIANTS makes nets.BoxPcLoss.emit set: checked here, where no GPU is needed."""
    import test_kernels_glue_gpu as G
    import test_off_recipe_cpu as T
    for over in T.BOXPC_VARIANTS:
        sw = (int(over.get('BOXPC_WEIGH_DELTA_LOSS_BY_CLS_CONF', False)), 0, int(over.get('BOXPC_WEIGH_DELTA_PRED_BY_CLS_CONF', False)),
              int(not over.get('BOXPC_STOP_GRAD_OF_CLS_VIA_DELTA', True)), int(over.get('BOXPC_DELTA_LOSS_TYPE', 'huber') == 'mse'))
        assert sw in G.LOSS_SWITCHES, over
