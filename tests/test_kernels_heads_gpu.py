"""GPU: the launch forms of the segmentation head, the box losses, the stage-c glue and the optimiser / element-wise kernels (csrc/heads.hip,
the second half of csrc/boxpc.hip, csrc/bn_optim.hip, csrc/weak.hip) that tests/test_kernels_gpu.py runs at one shape only: the cases of
tests/heads_check.py on libt3d.so, each against the fp64 specification (tests/fake_t3d.py) on identical seeded inputs, one launch per
comparison, every output NaN-filled and fenced by guard bands.  tests/test_kernels_heads_cpu.py runs the same cases on the specification
library and holds the host-only checks (seg-head decision margins, planted rows, the spec's backward against autograd of the oracle).

MEASURED_WORST (one run of this module on the MI355X, 177 passed in 5 s; against the fp64 specification, never against another run of a kernel;
per output, over its cases: the largest error `_within` prints, the bound at that element in brackets, the largest `error / bound` and the
case it came from.  No bound follows a measurement: they are the tolerances of the one-shape tests of tests/test_kernels_gpu.py, the 2e-5 of
the IoU tests, n_slabs 2^-24 sum|slab| for the slab sums and half a bf16 spacing for the stored bf16 dz, which a value just above a power of
two uses almost fully: 0.959.  Bit-for-bit comparisons -- the hard mask, part[:, 1:5] and part[:, 7] of t3d_seg_head, t3d_dropout_mask,
t3d_cast_bf16, untouched rows and columns, guard bands -- have no line.)
  strong_loss dbox                             4.876e-09  (3.491e-06)  0.003   B=128 iou=0 seg=0 norm3d=1 ld=72
  strong_loss dstage1                          3.363e-08  (5.638e-06)  0.006   B=1 iou=1 seg=1 norm3d=0 ld=67
  strong_loss terms                            1.722e-07  (1.271e-05)  0.014   B=1 iou=0 seg=0 norm3d=1 ld=72
  strong_loss total_losses                     1.362e-06  (2.980e-03)  0.001   B=1024 iou=1 seg=1 norm3d=0 ld=67
  strong_loss loss                             1.988e-07  (3.160e-04)  0.001   B=128 iou=0 seg=0 norm3d=1 ld=72
  strong_loss center                           1.192e-07  (2.713e-04)  0.000   B=513 iou=1 seg=1 norm3d=0 ld=67
  strong_loss reg_dims                         2.229e-07  (5.158e-04)  0.000   B=512 iou=1 seg=1 norm3d=0 ld=67
  strong_loss reg_theta                        4.768e-07  (5.841e-04)  0.001   B=512 iou=1 seg=1 norm3d=0 ld=67
  strong_loss iou3d                            5.162e-07  (2.000e-05)  0.026   B=1024 iou=1 seg=1 norm3d=0 ld=67
  strong_loss box_head_iou iou3d               6.474e-07  (2.000e-05)  0.032   B=513 iou=1 seg=1 norm3d=0 ld=67
  strong_loss iou3d against box_head_iou       6.780e-07  (2.000e-05)  0.034   B=513 iou=1 seg=1 norm3d=0 ld=67
  strong_loss iou2d                            6.769e-07  (2.000e-05)  0.034   B=128 iou=1 seg=1 norm3d=0 ld=67
  strong_loss box_head_iou iou2d               3.931e-06  (2.000e-05)  0.197   B=513 iou=1 seg=1 norm3d=0 ld=67
  strong_loss iou2d against box_head_iou       4.143e-06  (2.000e-05)  0.207   B=513 iou=1 seg=1 norm3d=0 ld=67
  box_head_iou iou3d                           2.980e-07  (2.000e-05)  0.015   B=200 ld=67 s1=1
  box_head_iou iou2d                           4.768e-07  (2.000e-05)  0.024   B=200 ld=67 s1=1
  dgrad_narrow f32 out                         6.104e-05  (1.837e-02)  0.003   M=192 N=384 k0=4 kn=6 ld=8
  dgrad_narrow bf16 out                        6.104e-05  (1.837e-02)  0.003   M=192 N=384 k0=4 kn=6 ld=8
  semi_final_loss d_dims                       2.910e-10  (1.007e-06)  0.000   B=7 only2d=0 default
  semi_final_loss dout9                        7.451e-09  (1.700e-06)  0.004   B=7 only2d=0 default
  semi_final_loss fit_prob                     1.192e-07  (7.022e-06)  0.018   B=1024 only2d=0 default
  semi_final_loss terms                        1.192e-07  (1.583e-05)  0.008   B=7 only2d=0 default
  semi_final_loss loss                         4.768e-07  (4.165e-05)  0.011   B=32 only2d=1 w_weak0
  anchor_reg_bwd dbox                          4.768e-07  (4.160e-05)  0.054   B=1024 ld=67 dbox7=1 d_dims=1
  anchor_reg_bwd dstage1                       0.000e+00  (1.319e-06)  0.000   B=1 ld=67 dbox7=1 d_dims=1
  seg_head f32 logits                          9.537e-07  (7.939e-05)  0.027   B=3 rpf=256 ld_pc=4 train_gen
  seg_head f32 part[:, 0|5|6]                  3.052e-05  (1.693e-02)  0.002   B=3 rpf=256 ld_pc=4 train_gen
  seg_head bf16 logits                         9.537e-07  (7.939e-05)  0.027   B=3 rpf=256 ld_pc=4 train_gen
  seg_head bf16 part[:, 0|5|6]                 3.052e-05  (1.693e-02)  0.002   B=3 rpf=256 ld_pc=4 train_gen
  seg_head f32 dz                              6.985e-10  (2.685e-07)  0.047   B=1 rpf=128 ld_pc=3 train_mask
  seg_head f32 psum_dz                         2.794e-09  (5.183e-06)  0.002   B=1 rpf=128 ld_pc=3 train_gen
  seg_head f32 psum_dzy                        3.725e-09  (2.286e-05)  0.002   B=1 rpf=128 ld_pc=3 train_gen
  seg_head f32 dw_part                         1.490e-08  (9.838e-05)  0.003   B=1 rpf=128 ld_pc=3 train_mask
  seg_head bf16 dz (bf16)                      7.178e-06  (8.780e-06)  0.959   B=1 rpf=128 ld_pc=3 train_nodrop
  seg_head bf16 psum_dz                        4.657e-10  (8.618e-06)  0.000   B=3 rpf=256 ld_pc=4 train_mask
  seg_head bf16 psum_dzy                       4.336e-09  (3.366e-05)  0.000   B=1 rpf=128 ld_pc=3 train_nodrop
  seg_head bf16 dw_part                        1.490e-08  (9.838e-05)  0.003   B=1 rpf=128 ld_pc=3 train_mask
  seg_finalize mask_xyz_mean                   0.000e+00  (4.388e-06)  0.000   B=1 tpf=1 given=1
  seg_finalize seg_loss                        0.000e+00  (4.156e-06)  0.000   B=1 tpf=1 given=1
  seg_finalize dw                              0.000e+00  (1.011e-05)  0.000   B=1 tpf=1 given=1
  seg_finalize dbias                           0.000e+00  (1.146e-05)  0.000   B=1 tpf=1 given=1
  seg_finalize n_correct                       0.000e+00  (8.210e-04)  0.000   B=1 tpf=1 given=1
  seg_finalize mean of the empty frustum       5.960e-08  (1.530e-05)  0.004   B=3 tpf=2 given=1
  reduce_slabs                                 1.833e-06  (6.187e-06)  0.405   max_numel=40004 slabs=9 numel=40004 mis=0
  optimiser w                                  4.768e-07  (4.263e-06)  0.264   n=524291
  optimiser v                                  2.478e-11  (1.937e-10)  0.130   n=524291
  optimiser m                                  1.863e-09  (6.626e-09)  0.345   n=524291
  optimiser wm                                 1.192e-07  (1.367e-06)  0.095   n=524291
  optimiser acc                                7.451e-09  (4.646e-08)  0.160   n=524291
  schedule_step                                0.000e+00  (2.500e-02)  0.000   from 24996
  weak_loss reproj                             1.526e-04  (2.000e-01)  0.001   B=65 N=128 both
  weak_loss surface                            2.980e-08  (5.326e-06)  0.006   B=256 N=128 both
  weak_loss dsoft                              3.274e-11  (9.162e-10)  0.036   B=256 N=128 both
  weak_loss total_losses                       9.537e-07  (1.022e-03)  0.001   B=256 N=128 both
  weak_loss loss                               4.768e-07  (2.590e-04)  0.002   B=65 N=128 both
  weak_loss dbox7                              1.099e-07  (1.009e-05)  0.011   B=256 N=128 both

FORM COVERAGE (kernel form -> test ids of this module)
  k_strong_loss<true> (B <= 128: heads and gradients in LDS; summary on thread 512 + f)                                              test_strong_loss[1-*], [128-*], test_strong_loss_argument_branches[64-*]
  k_strong_loss<false>, 128 < B <= 512 (private gradient, summary on thread 512 + f)                                                 test_strong_loss[129-*], [512-*], test_strong_loss_argument_branches[129-*]
  k_strong_loss<false>, B > 512 (summary inline)                                                                                     test_strong_loss[513-*], [1024-*]
  k_strong_loss without IoU outputs / without seg_loss / normalize_by_3d_count / ld_box 72                                           test_strong_loss[*-short], test_strong_loss_argument_branches
  k_strong_loss all-2-D batch (1e-3 guard)                                                                                           test_strong_loss_all_2d_batch
  k_box_head_iou: one 64-thread block, a partial block, several blocks; stage1_center NULL                                           test_box_head_iou
  k_dgrad_narrow: one / two / three column chunks, one / both accumulators, fp32 and bf16 dy                                         test_dgrad_narrow
  k_semi_final_loss: B below the class count, one full workgroup, T = 0, w_weak = 0, empty / single-member class, soft tie           test_semi_final_loss
  k_anchor_reg_bwd: optional pointers, accumulation, clamp, ties, ld_box 72                                                          test_anchor_reg_bwd
  k_seg_head<float> / <bf16_t>: infer, labels, train (no dropout, stored mask, generated mask), oracle_mask, exact ties              test_seg_head
  k_seg_head<float, true> / <bf16_t, true> (dsoft)                                                                                   test_seg_head[*-dsoft-*]
  k_seg_finalize: stride-256 loops over frustums (257, 300) and tiles (900, 640), empty mask, optional outputs                       test_seg_finalize
  reduce_slabs_body: 8-, 32- and 64-slab loops alone and chained, scalar path, misaligned slab_off, grid cap 256, small max_numel    test_reduce_slabs
  k_adam_tf / k_momentum_tf: one thread, part of a block, two blocks, the 2048-block cap                                             test_adam_and_momentum
  k_dropout_mask: the 4096-block cap, keep 1 and 1e-3, step 2^24, seed with the top bit                                              test_dropout_mask
  k_cast_bf16: vector body, scalar tail, grid-stride loop, alignment refusal                                                         test_cast_bf16, test_cast_bf16_refusals
  k_schedule_step: both staircases, step_offset                                                                                      test_schedule_step
  k_weak_surface / k_weak_finish: B = 1, 65, 256 (tot[256] full), 16 tiles per frustum, optional inputs                              test_weak_loss
"""
import pytest

import heads_check as hc

pytestmark = pytest.mark.gpu


@pytest.fixture
def env(hip_lib):
    return hc.Env(hip_lib, 'cuda')


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
