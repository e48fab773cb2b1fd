"""The head / loss / optimiser kernel cases of tests/heads_check.py on the executable specification (fake_t3d.FakeLib): the same functions
tests/test_kernels_heads_gpu.py runs on the device, so the cases (inputs, guard bands, refusals, planted rows) are validated without one --
plus what only the host can check: that every seg-head case keeps its decision margin, that the rows left out of the strong-loss
autograd comparison are the planted ones, and the specification's hand-derived strong-loss backward against autograd of the oracle."""
import pytest

import heads_check as hc
from fake_t3d import FakeLib


@pytest.fixture
def env():
    return hc.Env(FakeLib(), 'cpu')


# ---- 1. strong loss ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['full', 'short'])
@pytest.mark.parametrize('B', hc.STRONG_B)
def test_strong_loss(env, B, form):
    hc.check_strong_loss(env, B, *((True, True, 0, 67) if form == 'full' else (False, False, 1, 72)))


@pytest.mark.parametrize('B', [64, 129])
def test_strong_loss_argument_branches(env, B):
    for with_iou in (True, False):
        for with_seg in (True, False):
            for norm3d in (0, 1):
                for ld in (67, 72):
                    hc.check_strong_loss(env, B, with_iou, with_seg, norm3d, ld)


@pytest.mark.parametrize('B', [64, 129])
def test_strong_loss_all_2d_batch(env, B):
    hc.check_strong_loss(env, B, True, True, 1, 67, all2d=True)


def test_strong_loss_refusals(env):
    hc.check_strong_refusals(env)


@pytest.mark.parametrize('B', [64, 129])
def test_strong_loss_planted_rows_are_what_they_claim(B):
    zero, flip = hc.strong_case_facts(B)
    assert sorted(zero.tolist()) == sorted(hc.ZERO_ROWS)
    assert (flip > 0.5).all(), 'the flipped corner set does not win on every corner'


@pytest.mark.parametrize('norm3d', [0, 1])
@pytest.mark.parametrize('B', [64, 129])
def test_strong_loss_spec_backward_against_autograd(B, norm3d):
    hc.check_strong_spec_against_autograd(B, norm3d)


@pytest.mark.parametrize('B,ld,with_s1', [(B, 67, True) for B in hc.HEAD_IOU_B] + [(65, 72, True), (200, 72, False), (63, 67, False)])
def test_box_head_iou(env, B, ld, with_s1):
    hc.check_box_head_iou(env, B, ld, with_s1)


def test_box_head_iou_refusals(env):
    hc.check_box_head_iou_refusals(env)


# ---- 2. stage-c glue ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('M,N,k0,kn,ld_out', hc.NARROW_SHAPES)
def test_dgrad_narrow(env, M, N, k0, kn, ld_out, bf16):
    hc.check_dgrad_narrow(env, M, N, k0, kn, ld_out, bf16)


def test_dgrad_narrow_refusals(env):
    hc.check_dgrad_narrow_refusals(env)


@pytest.mark.parametrize('variant', ['default', 'w_weak0', 'T0'])
@pytest.mark.parametrize('only2d', [0, 1])
@pytest.mark.parametrize('B', hc.SEMI_B)
def test_semi_final_loss(env, B, only2d, variant):
    hc.check_semi_final_loss(env, B, only2d, variant)


@pytest.mark.parametrize('with7,with_dd', [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize('ld', [67, 72])
@pytest.mark.parametrize('B', hc.ANCHOR_B)
def test_anchor_reg_bwd(env, B, ld, with7, with_dd):
    hc.check_anchor_reg_bwd(env, B, ld, with7, with_dd)


def test_anchor_reg_bwd_refusals(env):
    hc.check_anchor_reg_bwd_refusals(env)


# ---- 3. seg head ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', hc.SEG_FORMS)
@pytest.mark.parametrize('B,rpf,ld_pc', hc.SEG_SHAPES)
def test_seg_head_cases_keep_their_decision_margin(B, rpf, ld_pc, form):
    hc.check_seg_margin(B, rpf, form)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('form', hc.SEG_FORMS)
@pytest.mark.parametrize('B,rpf,ld_pc', hc.SEG_SHAPES)
def test_seg_head(env, B, rpf, ld_pc, form, bf16):
    hc.check_seg_head(env, B, rpf, ld_pc, form, bf16)


@pytest.mark.parametrize('given', [1, 0])
@pytest.mark.parametrize('B,tpf', hc.FINALIZE_SHAPES)
def test_seg_finalize(env, B, tpf, given):
    hc.check_seg_finalize(env, B, tpf, given)


# ---- 4. optimiser and element-wise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_numel', [40004, 640])
def test_reduce_slabs(env, max_numel):
    hc.check_reduce_slabs(env, max_numel)


@pytest.mark.parametrize('n', hc.OPT_N)
def test_adam_and_momentum(env, n):
    hc.check_adam_and_momentum(env, n)


@pytest.mark.parametrize('n', hc.MASK_N)
def test_dropout_mask(env, n):
    hc.check_dropout_mask(env, n)


@pytest.mark.parametrize('n', hc.CAST_N)
def test_cast_bf16(env, n):
    hc.check_cast_bf16(env, n)


def test_cast_bf16_refusals(env):
    hc.check_cast_bf16_refusals(env)


def test_schedule_step(env):
    hc.check_schedule_step(env)


# ---- 5. weak loss shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,form', [(B, N, 'both') for B, N in hc.WEAK_SHAPES] + [(65, 128, f) for f in hc.WEAK_FORMS[1:]])
def test_weak_loss(env, B, N, form):
    hc.check_weak_loss(env, B, N, form)


def test_weak_loss_refusals(env):
    hc.check_weak_loss_refusals(env)


def test_gpu_module_docstring_carries_the_form_table():
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_kernels_heads_gpu.py')).read()
    assert hc.forms_text() in text, 'tests/test_kernels_heads_gpu.py: its FORM COVERAGE table is not heads_check.forms_text()'
