"""ctypes view of include/t3d.h: argument structs + loader for libt3d.so.

The product path has no fallback: `load()` raises if the HIP library is missing or does not export
every entry point the header declares.
"""
import ctypes as C
import os

F = C.POINTER(C.c_float)
I = C.POINTER(C.c_int32)
D = C.POINTER(C.c_double)
L = C.POINTER(C.c_int64)
i32, f32 = C.c_int, C.c_float

TILE_ROWS = 128
F32, BF16 = 0, 1              # t3d.h: T3D_F32 / T3D_BF16 (element type of the per-point layer tensors + GEMM arithmetic)
DTYPE_BY_NAME = {'f32': F32, 'bf16': BF16}
ARITH_AUTO, ARITH_FP32_MFMA, ARITH_BF16X3, ARITH_BF16 = 0, 1, 2, 3      # t3d.h: T3D_ARITH_* (arithmetic of an fp32 GEMM launch)
ARITH_BY_NAME = {'auto': ARITH_AUTO, 'fp32_mfma': ARITH_FP32_MFMA, 'bf16x3': ARITH_BF16X3}
ARITH_NAMES = {ARITH_FP32_MFMA: 'fp32_mfma', ARITH_BF16X3: 'bf16x3', ARITH_BF16: 'bf16'}
ABI_VERSION = 3
ERR_ABI = -4
ACT_NONE, ACT_RELU, ACT_LEAKY_RELU, ACT_TANH = 0, 1, 2, 3
ACT_BY_NAME = {None: ACT_NONE, 'relu': ACT_RELU, 'leaky_relu': ACT_LEAKY_RELU, 'tanh': ACT_TANH}


class Sized(C.Structure):
    """An argument struct of ABI version 2 that starts with `struct_size` (t3d.h): filled in here, so positional construction
    keeps listing the fields behind it."""

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(type(self)), *args, **kw)


class ActSrc(C.Structure):
    _fields_ = [('x', F), ('ldx', i32), ('coff', i32), ('scale', F), ('shift', F), ('relu', i32),
                ('sub', F), ('sub_ld', i32), ('dtype', i32)]


class DySrc(C.Structure):
    _fields_ = [('dz', F), ('y', F), ('coef', F), ('argidx', I), ('dpool', F), ('dtype', i32)]


class PointMlpFwdArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('a', ActSrc), ('w', F), ('bias', F), ('rowbias', F), ('y', F), ('psum', F), ('psumsq', F),
                ('rowmask', F), ('pmax', F), ('pmin', F), ('pamax', I), ('pamin', I),
                ('M', i32), ('K', i32), ('N', i32), ('rows_per_frustum', i32), ('dtype', i32), ('w_x3', C.c_void_p), ('w_x3_stride', C.c_int64), ('arith', i32)]


class BnFwdFinalizeArgs(C.Structure):
    _fields_ = [('psum', F), ('psumsq', F), ('n_tiles', i32), ('count', i32), ('N', i32), ('gamma', F), ('beta', F),
                ('moving_mean', F), ('moving_var', F), ('decay', F), ('eps', f32), ('is_training', i32),
                ('unbiased_ema', i32), ('scale', F), ('shift', F), ('mean', F), ('invstd', F),
                ('pool_pmax', F), ('pool_pmin', F), ('pool_pamax', I), ('pool_pamin', I), ('pool_B', i32), ('pool_tiles_per_frustum', i32),
                ('pooled', F), ('ld_pooled', i32), ('argidx', I), ('ysel', F)]


class PoolFinalizeArgs(C.Structure):
    _fields_ = [('scale', F), ('shift', F), ('pmax', F), ('pmin', F), ('pamax', I), ('pamin', I),
                ('B', i32), ('N', i32), ('tiles_per_frustum', i32), ('pooled', F), ('ld_pooled', i32),
                ('argidx', I), ('ysel', F)]


class PointMlpDgradArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('dy', DySrc), ('w', F), ('add_in', F), ('prev_y', F), ('prev_scale', F), ('prev_shift', F),
                ('out', F), ('psum_dz', F), ('psum_dzy', F), ('M', i32), ('K', i32), ('N', i32),
                ('rows_per_frustum', i32), ('dtype', i32), ('w_x3', C.c_void_p), ('w_x3_stride', C.c_int64), ('arith', i32)]


class PointMlpWgradArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('a', ActSrc), ('dy', DySrc), ('slabs', F), ('M', i32), ('K', i32), ('N', i32),
                ('rows_per_frustum', i32), ('rows_per_split', i32), ('arith', i32)]


class PoolBwdPrepArgs(C.Structure):
    _fields_ = [('w', F), ('bias', F), ('coef', F), ('K', i32), ('N', i32), ('p_slabs', F), ('rc_slabs', F), ('wc', F)]


class PoolSparseRowsArgs(C.Structure):
    _fields_ = [('argidx', I), ('dpool', F), ('wc', F), ('B', i32), ('N', i32), ('K', i32), ('rows_per_frustum', i32), ('s', F),
                ('row_live', I)]


class PointMlpDgradGramArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('a', ActSrc), ('p', F), ('rowconst', F), ('add_in', F), ('add_live', I), ('prev_y', F), ('prev_scale', F),
                ('prev_shift', F),
                ('out', F), ('psum_dz', F), ('psum_dzy', F), ('M', i32), ('K', i32), ('rows_per_frustum', i32), ('dtype', i32), ('arith', i32)]


class PointMlpGramArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('a', ActSrc), ('slabs', F), ('M', i32), ('K', i32), ('rows_per_frustum', i32), ('rows_per_split', i32), ('arith', i32)]


class ActColsumArgs(C.Structure):
    _fields_ = [('a', ActSrc), ('M', i32), ('K', i32), ('rows_per_frustum', i32), ('part', F)]


class PoolWgradFinishArgs(C.Structure):
    _fields_ = [('a', ActSrc), ('argidx', I), ('dpool', F), ('coef', F), ('w', F), ('bias', F), ('g', F), ('abar', F),
                ('B', i32), ('K', i32), ('N', i32), ('rows_per_frustum', i32), ('dw', F)]


class BoxRefineStepArgs(C.Structure):
    _fields_ = [('out9', F), ('center_in', F), ('dims_in', F), ('theta_in', F), ('center_out', F), ('dims_out', F), ('theta_out', F),
                ('total', F), ('fit_prob', F), ('weigh_by_conf', i32), ('first', i32), ('B', i32)]


class ClassGroups(C.Structure):
    _fields_ = [('members', I), ('offsets', I), ('n_groups', i32), ('perm', I), ('perm_len', i32)]


class SampleEqualClassesArgs(C.Structure):
    _fields_ = [('set', ClassGroups * 2), ('B', i32), ('seed', C.c_uint32), ('hyper', F), ('order_draws', F), ('member_draws', F),
                ('equal_prob', f32), ('prob_draw', F), ('sample', I), ('is_data_2D', I)]


class BoxPcPerturbArgs(C.Structure):
    _fields_ = [('center', F), ('orient_cls', I), ('orient_reg', F), ('dims_cls', I), ('dims_reg', F), ('y_box_iou', F),
                ('y_center_delta', F), ('y_dims_delta', F), ('y_orient_delta', F), ('center_perturbation', f32),
                ('size_perturbation', f32), ('angle_perturbation', f32), ('fit_lo', f32), ('fit_hi', f32), ('nofit_lo', f32),
                ('nofit_hi', f32), ('proportion_fit', f32), ('fit_draw', F), ('cand_draws', F), ('max_rounds', i32),
                ('seed', C.c_uint32), ('hyper', F), ('B', i32)]


class Box3dIouArgs(C.Structure):
    _fields_ = [('center1', F), ('size1', F), ('heading1', F), ('center2', F), ('size2', F), ('heading2', F), ('iou3d', F), ('iou2d', F),
                ('n', i32)]


class Box3dIouCornersArgs(C.Structure):
    _fields_ = [('corners1', F), ('corners2', F), ('iou3d', F), ('iou2d', F), ('n', i32)]


class BoxHeadIouArgs(C.Structure):
    _fields_ = [('box', F), ('ld_box', i32), ('stage1_center', F), ('y_center', F), ('y_orient_cls', I), ('y_orient_reg', F),
                ('y_dims_cls', I), ('y_dims_reg', F), ('iou2d', F), ('iou3d', F), ('B', i32)]


class BatchAssembleArgs(C.Structure):
    _fields_ = [('points', F), ('seg', I), ('offsets', C.POINTER(C.c_int64)), ('frustum_angle', F), ('box_center', F), ('heading', F),
                ('size', F), ('cls', I), ('sample', I), ('sample_len', i32), ('choice', I), ('aug', F), ('C_src', i32), ('C', i32), ('B', i32), ('N', i32),
                ('rotate_to_center', i32), ('random_flip', i32), ('random_shift', i32), ('seed', C.c_uint32), ('hyper', F), ('pc', F),
                ('y_seg', I), ('y_center', F), ('y_orient_cls', I), ('y_orient_reg', F), ('y_dims_cls', I), ('y_dims_reg', F),
                ('one_hot', F), ('rot_angle', F), ('sample2', I), ('sample2_len', i32), ('is_data_2D', I), ('frustum_is_2D', I), ('ld_pc', i32),
                ('slot_is_2D', I), ('cam_rtilt', F), ('cam_k', F), ('cam_box2d', F), ('cam_img_dim', F), ('Rtilt', F), ('K', F), ('box2D', F),
                ('img_dim', F)]


class BnBwdFinalizeArgs(C.Structure):
    _fields_ = [('psum_dz', F), ('psum_dzy', F), ('n_tiles', i32), ('dpool_in', F), ('ld_dpool_in', i32),
                ('pooled', F), ('ld_pooled', i32), ('ysel', F), ('dpool', F), ('B', i32), ('count', i32), ('N', i32),
                ('gamma', F), ('mean', F), ('invstd', F), ('scale', F), ('frozen', i32), ('dgamma', F), ('dbeta', F),
                ('coef', F)]


class DyColsumArgs(C.Structure):
    _fields_ = [('psum_dz', F), ('psum_y', F), ('coef', F), ('B', i32), ('N', i32), ('tiles_per_frustum', i32),
                ('rows_per_frustum', i32), ('alpha', f32), ('out', F)]


class FcFwdArgs(C.Structure):
    _fields_ = [('in_', F), ('ld_in', i32), ('K', i32), ('in2', F), ('ld_in2', i32), ('K2', i32), ('w', F), ('bias', F),
                ('gamma', F), ('beta', F), ('moving_mean', F), ('moving_var', F), ('decay', F), ('eps', f32),
                ('is_training', i32), ('unbiased_ema', i32), ('act', i32), ('leaky_alpha', f32), ('drop_mask', F),
                ('keep_prob', f32), ('add_in', F), ('ld_add', i32), ('add_n', i32), ('y', F), ('out', F),
                ('ld_out', i32), ('mean', F), ('invstd', F), ('B', i32), ('N', i32)]


class FcBwdArgs(C.Structure):
    _fields_ = [('dout', F), ('ld_dout', i32), ('dy_next', F), ('w_next', F), ('N_next', i32),
                ('in_', F), ('ld_in', i32), ('K', i32), ('in2', F), ('ld_in2', i32), ('K2', i32),
                ('y', F), ('out', F), ('ld_out', i32), ('gamma', F), ('beta', F), ('mean', F), ('invstd', F),
                ('bn_training', i32), ('act', i32), ('leaky_alpha', f32), ('drop_mask', F), ('keep_prob', f32),
                ('dy', F), ('dw', F), ('dbias', F), ('dgamma', F), ('dbeta', F), ('B', i32), ('N', i32)]


class FcDinputArgs(C.Structure):
    _fields_ = [('dy', F), ('N', i32), ('w', F), ('add_in', F), ('ld_add', i32), ('alpha', f32), ('din', F),
                ('ld_din', i32), ('B', i32), ('K', i32),
                ('bn_pooled', F), ('bn_ld_pooled', i32), ('bn_ysel', F), ('bn_dpool', F), ('bn_count', i32), ('bn_gamma', F), ('bn_mean', F),
                ('bn_invstd', F), ('bn_scale', F), ('bn_frozen', i32), ('bn_dgamma', F), ('bn_dbeta', F), ('bn_coef', F)]


class SegHeadArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('y', F), ('scale', F), ('shift', F), ('drop_mask', F), ('keep_prob', f32), ('w', F), ('bias', F),
                ('labels', I), ('is_data_2D', I), ('pc', F), ('ld_pc', i32), ('ce_weight', f32), ('logits', F),
                ('mask', F), ('part', F), ('dz', F), ('psum_dz', F), ('psum_dzy', F), ('dw_part', F),
                ('M', i32), ('K', i32), ('rows_per_frustum', i32), ('B', i32), ('drop_seed', C.c_uint32), ('drop_hyper', F),
                ('dtype', i32), ('dsoft', F), ('oracle_mask', I)]


SMALL_KIND = {'t3d_bn_bwd_finalize': 1, 't3d_fc_bwd': 2, 't3d_fc_dinput': 3, 't3d_dy_colsum': 4}      # t3d.h T3D_SMALL_* (t3d_small_pair)
RIDER_KIND = dict(SMALL_KIND, t3d_bn_fwd_finalize=5, t3d_fc_fwd=6, t3d_pool_bwd_mid=7)                  # kinds a rider set takes
RIDER_FIELD = {1: 'bn_bwd', 2: 'fc_bwd', 3: 'fc_dinput', 4: 'dy_colsum', 5: 'bn_fwd', 6: 'fc_fwd', 7: 'mid'}
RIDER_WIDE = ('t3d_pool_bwd_mid',)      # hundreds of workgroups, alone in its set


class WeakLossArgs(C.Structure):
    _fields_ = [('center', F), ('reg_dims', F), ('reg_theta', F), ('pc', F), ('ld_pc', i32), ('logits', F), ('Rtilt', F), ('K', F),
                ('rot_frust', F), ('box2D', F), ('img_dim', F), ('is_data_2D', I), ('w_reproj', f32), ('w_surface', f32),
                ('multiplier', f32), ('use_softmax_proj', i32), ('softmax_scale', f32), ('dilate', f32), ('clip_lower_b_loss', i32),
                ('clip_pred_box', i32), ('loss_mse', i32), ('train_box_reproj', i32 * 3), ('train_box_surface', i32 * 3),
                ('surface_margin', f32), ('surface_scale_dims', f32), ('surf_part', F), ('dsoft', F), ('reproj', F), ('surface', F),
                ('dbox7', F), ('total_losses', F), ('loss', F), ('B', i32), ('N', i32), ('one_hot', F), ('w_inactive', f32),
                ('inactive_margins', f32 * 10), ('inactive_train', i32 * 10), ('inactive', F)]


class ActDropoutArgs(C.Structure):
    _fields_ = [('a', ActSrc), ('mask', F), ('keep_prob', f32), ('out', F), ('M', i32), ('K', i32), ('rows_per_frustum', i32)]


class SegFinalizeArgs(C.Structure):
    _fields_ = [('part', F), ('dw_part', F), ('B', i32), ('tiles_per_frustum', i32), ('rows_per_frustum', i32),
                ('K', i32), ('mask_xyz_mean', F), ('seg_loss', F), ('dw', F), ('dbias', F), ('n_correct', F)]


class StrongWeights(C.Structure):
    _fields_ = [(n, f32) for n in ('center', 'orient_cls', 'orient_reg', 'dims_cls', 'dims_reg', 'tnet_center',
                                   'corner', 'box_multiplier', 'cross_entropy')]


class StrongLossArgs(C.Structure):
    _fields_ = [('box', F), ('ld_box', i32), ('stage1_center', F), ('seg_loss', F), ('y_center', F),
                ('y_orient_cls', I), ('y_orient_reg', F), ('y_dims_cls', I), ('y_dims_reg', F), ('is_data_2D', I),
                ('wts', StrongWeights), ('normalize_by_3d_count', i32), ('dbox', F), ('dstage1', F), ('terms', F),
                ('total_losses', F), ('loss', F), ('center', F), ('reg_dims', F), ('reg_theta', F), ('iou2d', F), ('iou3d', F), ('B', i32)]


class X3FragEntry(C.Structure):      # t3d_x3_frag_entry (t3d_split_x3_frag)
    _fields_ = [('off', C.c_int64), ('K', C.c_int32), ('N', C.c_int32), ('fwd', C.c_int32), ('dgrad', C.c_int32), ('blk0', C.c_int32), ('reserved', C.c_int32)]


def x3_frag_table(entries):
    """(bytes of a t3d_x3_frag_entry table as a NumPy uint8 array, number of workgroups) for [(off, K, N), ...] (both arrangements)"""
    import numpy as np
    rec = np.zeros(len(entries), dtype=np.dtype([('off', '<i8'), ('K', '<i4'), ('N', '<i4'), ('fwd', '<i4'), ('dgrad', '<i4'), ('blk0', '<i4'), ('reserved', '<i4')]))
    blk = 0
    for i, (off, K, N) in enumerate(entries):
        rec[i] = (off, K, N, 1, 1, blk, 0)
        blk += (K * N // 8 + 255) // 256
    return rec.view(np.uint8).copy(), blk


class SlabDesc(C.Structure):
    _fields_ = [('slab_off', C.c_int64), ('grad_off', C.c_int64), ('numel', C.c_int32), ('n_slabs', C.c_int32)]


class AdamRange(C.Structure):      # t3d_adam_range (t3d_reduce_slabs_adam)
    _fields_ = [('off', C.c_int64), ('n', C.c_int64), ('blk0', C.c_int32), ('reserved', C.c_int32)]


ADAM_RANGE_ELEMS = 1024      # elements per workgroup of a range (csrc/bn_optim.hip)


def adam_range_table(n_total, slab_tensors):
    """([(off, n, blk0), ...], number of workgroups): the ranges of [0, n_total) that no slab tensor [(grad_off, numel), ...] covers.
    Raises unless the slab tensors lie inside [0, n_total) and do not overlap -- with the ranges they then partition it, so that
    t3d_reduce_slabs_adam updates every element exactly once."""
    out, pos, blk = [], 0, 0
    for off, n in sorted(slab_tensors):
        if n <= 0 or off < pos or off + n > n_total:
            raise T3DError('slab tensors overlap or leave the parameter buffer: (%d, %d) after %d of %d' % (off, n, pos, n_total))
        if off > pos:
            out.append((pos, off - pos, blk))
            blk += (off - pos + ADAM_RANGE_ELEMS - 1) // ADAM_RANGE_ELEMS
        pos = off + n
    if pos < n_total:
        out.append((pos, n_total - pos, blk))
        blk += (n_total - pos + ADAM_RANGE_ELEMS - 1) // ADAM_RANGE_ELEMS
    assert sum(n for _, n, _ in out) + sum(n for _, n in slab_tensors) == n_total
    return out, blk


class Schedule(C.Structure):
    _fields_ = [('base_lr', f32), ('lr_decay_rate', f32), ('lr_decay_step', f32), ('bn_init_decay', f32),
                ('bn_decay_rate', f32), ('bn_decay_step', f32), ('bn_decay_clip', f32), ('beta1', f32), ('beta2', f32),
                ('batch_size', i32), ('step_offset', i32)]


class BoxPcRepArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('pc', F), ('ld_pc', i32), ('C', i32), ('center', F), ('dims', F), ('theta', F), ('y_dims_cls', I),
                ('y_orient_cls', I), ('rep', F), ('ld_rep', i32), ('box_out', F), ('M', i32), ('rows_per_frustum', i32), ('rowmask', F)]


class BoxPcRepBArgs(C.Structure):
    _fields_ = [('center', F), ('dims', F), ('theta', F), ('y_dims_cls', I), ('y_orient_cls', I), ('box_out', F), ('pc', F), ('ld_pc', i32),
                ('C', i32), ('rowmask', F), ('pc_out', F), ('ld_out', i32), ('B', i32), ('rows_per_frustum', i32)]


class BoxPcRepBwdArgs(C.Structure):
    _fields_ = [('pc', F), ('ld_pc', i32), ('box', F), ('drep', F), ('ld_drep', i32), ('coff', i32), ('dbox', F),
                ('B', i32), ('rows_per_frustum', i32)]


class BoxPcLossArgs(C.Structure):
    _fields_ = [('out', F), ('y_box_iou', F), ('y_center_delta', F), ('y_dims_delta', F), ('y_orient_delta', F),
                ('fit_bound', f32), ('w_cls', f32), ('w_delta', f32), ('w_center', f32), ('w_size', f32), ('w_angle', f32),
                ('weigh_by_cls_conf', i32), ('weigh_by_cls_gt', i32), ('dout', F), ('terms', F), ('loss', F), ('B', i32),
                ('weigh_pred_by_cls_conf', i32), ('grad_cls_via_delta', i32), ('delta_loss_mse', i32)]


class BoxRefineStepBwdArgs(C.Structure):
    _fields_ = [('out9', F), ('dbox_rep', F), ('carry', F), ('tot_out', F), ('dout9', F), ('weigh_by_conf', i32),
                ('grad_via_conf', i32), ('B', i32)]


class Box2dFeatsArgs(C.Structure):
    _fields_ = [('one_hot', F), ('n_oh', i32), ('box2D', F), ('img_dim', F), ('out', F), ('B', i32)]


class DgradNarrowArgs(C.Structure):
    _fields_ = [('dy', DySrc), ('w', F), ('k0', i32), ('kn', i32), ('out', F), ('ld_out', i32), ('M', i32), ('N', i32)]


class SemiFinalLossArgs(C.Structure):
    _fields_ = [('strong_loss', F), ('reg_dims', F), ('one_hot', F), ('is_data_2D', I), ('out9', F),
                ('train_classes', C.c_int32 * 10), ('w_weak', f32), ('w_fit', f32), ('fit_only_2d', i32), ('d_dims', F),
                ('dout9', F), ('fit_prob', F), ('terms', F), ('loss', F), ('B', i32)]


class AnchorRegBwdArgs(C.Structure):
    _fields_ = [('box', F), ('ld_box', i32), ('dbox7', F), ('d_dims', F), ('dbox', F), ('dstage1', F), ('B', i32)]


class FrustumExtractArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('points', D), ('scene_offsets', L), ('rtilt', D), ('K', D), ('scene_jobs', I),
                ('n_scenes', i32), ('max_scene_points', i32), ('C_src', i32), ('C', i32), ('n_jobs', i32), ('num_points', i32),
                ('box2d', D), ('perturb_box2d', i32), ('perturb_draws', D), ('box3d', D), ('job_key', I), ('seed', C.c_uint32),
                ('choice', I), ('mask_offsets', L), ('masks', C.POINTER(C.c_uint64)), ('seg_prefix', I), ('box2d_out', D),
                ('frustum_angle', D), ('n_in_box', I), ('count', I), ('index', I), ('out_points', D), ('label', I)]


U8 = C.POINTER(C.c_uint8)
VP_ = C.c_void_p              # a table of structs, passed as an address


class SunrgbdEvalArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('P', i32), ('G', i32), ('det_centroid', D), ('det_basis', D), ('det_coeffs', D),
                ('det_confidence', D), ('det_image', I), ('gt_centroid', D), ('gt_basis', D), ('gt_coeffs', D), ('gt_image', I),
                ('gt_difficult', U8), ('n_images', i32), ('image_ids', I), ('image_gt_offsets', I), ('image_gt', I),
                ('threshold', C.c_double), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64), ('order', I), ('max_overlap', D),
                ('gt_idx', I), ('is_tp', U8), ('is_fp', U8), ('gt_assignment', I), ('is_missed', U8), ('precision', D), ('recall', D),
                ('ap', D), ('overlap_offsets', L), ('overlaps', D), ('overlap_gt', I)]


DIAG_KINDS = ('tp', 'cls', 'loc', 'both', 'dup', 'bkg')                          # t3d.h T3D_DIAG_*: kind[i], counts[6]
DIAG_FIXES = ('cls', 'loc', 'both', 'dup', 'bkg', 'missed', 'fp', 'fn')         # t3d.h T3D_DIAG_FIX_*: ap_fixed[8]


class SunrgbdDiagnoseArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('Go', i32), ('other_centroid', D), ('other_basis', D), ('other_coeffs', D), ('other_image', I),
                ('n_other_images', i32), ('other_image_ids', I), ('other_image_offsets', I), ('other_image_list', I),
                ('bg_threshold', C.c_double), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64), ('other_overlap', D),
                ('other_gt', I), ('kind', U8), ('gt_state', U8), ('counts', I), ('gt_counts', I), ('ap_fixed', D)]


LOC_PARTS = ('xy', 'z', 'centre', 'size', 'heading')                             # t3d.h T3D_LOCPART_*: part_overlap[i][5], ap_part[5]
LOC_ERRORS = ('xy', 'z', 'l', 'w', 'h', 'heading')                               # loc_error[i][6]


class SunrgbdLocPartsArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('reserved', i32), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64),
                ('part_overlap', D), ('loc_error', D), ('part_counts', I), ('part_boxes', I), ('ap_part', D)]


# t3d.h T3D_RESCORE_*: the named features (bit k of feature_mask is RESCORE_FEATURES[k]), the limits and the status bits of the fit
RESCORE_FEATURES = ('logit_prob', 'score', 'reproj_iou', 'mask_in_box', 'seg_box_iou', 'log_mask', 'view_iou')
RESCORE_MAX_FEATURES, RESCORE_SLICE, RESCORE_MAX_HALVINGS = 15, 2048, 30
RESCORE_NO_ROWS, RESCORE_ONE_CLASS, RESCORE_CONSTANT_COLUMN, RESCORE_NOT_CONVERGED, RESCORE_NONFINITE = 1, 2, 4, 8, 16
RESCORE_STATUS = {RESCORE_NO_ROWS: 'no_rows', RESCORE_ONE_CLASS: 'one_class', RESCORE_CONSTANT_COLUMN: 'constant_column',
                  RESCORE_NOT_CONVERGED: 'not_converged', RESCORE_NONFINITE: 'nonfinite'}


class RescoreFeaturesArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('ld', i32), ('feature_mask', C.c_uint32), ('prob', F), ('score', F), ('reproj', D),
                ('counts', I), ('view_iou', F), ('X', D)]


class RescoreFitArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('F', i32), ('ld', i32), ('max_iter', i32), ('reserved', i32), ('X', D), ('y', U8),
                ('r', D), ('lambda_', C.c_double), ('gtol', C.c_double), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64),
                ('coef', D), ('coef_std', D), ('mean', D), ('scale', D), ('loss', D), ('n_iter', I), ('status', C.POINTER(C.c_uint32)),
                ('n_rows', L), ('n_pos', L)]


class RescoreApplyArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('n_valid', i32), ('F', i32), ('ld', i32), ('reserved', i32), ('X', D), ('coef', D),
                ('out', D), ('out32', F)]


SEMI_BATCH, SEMI_ALTERNATE_BATCH, SEMI_MIXED_BATCH = 0, 1, 2          # t3d.h T3D_SEMI_*
SEMI_METHODS = {'BATCH': SEMI_BATCH, 'ALTERNATE_BATCH': SEMI_ALTERNATE_BATCH, 'MIXED_BATCH': SEMI_MIXED_BATCH}
SEMI_SAMPLE_MAX_B = 256


class SemiList(C.Structure):
    _fields_ = [('ids', I), ('len', i32), ('members', I), ('offsets', I), ('n_groups', i32)]


class SemiSampleArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('method', i32), ('list3d', SemiList), ('list2d', SemiList), ('perm', I), ('perm_len', i32),
                ('B', i32), ('seed', C.c_uint32), ('equal_prob', f32), ('hyper', F), ('sample', I), ('is_data_2D', I)]


NUM_CLASS = 10                # t3d.h T3D_NUM_CLASS


class LabelSubsetArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('F', i32), ('cls', I), ('member', U8), ('class_mask', I), ('keep_prob', f32), ('add_prob', f32),
                ('seed', C.c_uint32), ('reserved', i32), ('ids', I), ('members', I), ('offsets', I), ('present', I), ('summary', I)]


class DetectDecodeArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('B', i32), ('N', i32), ('n_valid', i32), ('ld_box', i32), ('logits', F), ('box_out', F),
                ('stage1_center', F), ('total_delta', F), ('fit_prob', F), ('rot_angle', F), ('seg', U8), ('score', F), ('mask_count', I),
                ('heading_cls', I), ('size_cls', I), ('center', F), ('heading_res', F), ('size_res', F), ('label', F), ('corners', F)]


NMS_IOU3D, NMS_IOU2D = 0, 1           # t3d.h T3D_NMS_*
NMS_METRICS = {'3d': NMS_IOU3D, 'bev': NMS_IOU2D}
DETECT_NMS_MAX_GROUP = 1024           # t3d.h T3D_DETECT_NMS_MAX_GROUP


class DetectNmsArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('n_groups', i32), ('metric', i32), ('corners', F), ('score', F), ('group_offsets', I),
                ('members', I), ('threshold', f32), ('max_group', i32), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64), ('keep', U8),
                ('suppressed_by', I), ('rank', I)]


def detect_nms_workspace_bytes(n, max_group):
    """t3d.h T3D_DETECT_NMS_WORKSPACE_BYTES"""
    return (n + 1) // 2 * 8 + n * ((max_group + 63) // 64) * 8


SOFT_NMS_GAUSSIAN, SOFT_NMS_LINEAR = 0, 1       # t3d.h T3D_SOFT_NMS_*
SOFT_NMS_METHODS = {'gaussian': SOFT_NMS_GAUSSIAN, 'linear': SOFT_NMS_LINEAR}


class DetectSoftNmsArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('n_groups', i32), ('metric', i32), ('corners', F), ('score', F), ('group_offsets', I),
                ('members', I), ('threshold', f32), ('max_group', i32), ('method', i32), ('sigma', f32), ('min_score', f32), ('reserved', i32),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64), ('score_out', F), ('keep', U8), ('suppressed_by', I), ('n_decays', I)]


def detect_soft_nms_workspace_bytes(n, max_group):
    """t3d.h T3D_DETECT_SOFT_NMS_WORKSPACE_BYTES"""
    return 0


RENDER_RGB, RENDER_LABEL, RENDER_FLAT = 0, 1, 2      # t3d.h T3D_RENDER_*


class RenderView(C.Structure):
    _fields_ = [('P', f32 * 16), ('w_near', f32), ('H', i32), ('W', i32), ('pixel_first', i32), ('out_offset', C.c_int64),
                ('bg_offset', C.c_int64), ('bg_colour', f32 * 3), ('reserved', i32)]


class RenderPoints(C.Structure):
    _fields_ = [('view', i32), ('first', i32), ('count', i32), ('mode', i32), ('colour0', f32 * 3), ('colour1', f32 * 3), ('splat', i32),
                ('reserved', i32), ('pos_first', C.c_int64)]


class RenderBox(C.Structure):
    _fields_ = [('view', i32), ('box', i32), ('colour', f32 * 3), ('thickness', i32)]


class RenderRect(C.Structure):
    _fields_ = [('view', i32), ('xmin', f32), ('ymin', f32), ('xmax', f32), ('ymax', f32), ('colour', f32 * 3), ('thickness', i32)]


class RenderArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n_views', i32), ('n_points', i32), ('n_ranges', i32), ('n_corner_boxes', i32), ('n_boxes', i32),
                ('n_rects', i32), ('ld_xyz', i32), ('views', VP_), ('xyz', F), ('rgb', F), ('label', U8), ('ranges', VP_), ('corners', F),
                ('boxes', VP_), ('rects', VP_), ('total_pixels', C.c_int64), ('total_point_items', C.c_int64), ('bg', U8),
                ('bg_bytes', C.c_uint64), ('out', U8), ('out_bytes', C.c_uint64), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64),
                ('views_host', VP_), ('ranges_host', VP_), ('boxes_host', VP_), ('rects_host', VP_)]


def render_workspace_bytes(pixels):
    """t3d.h T3D_RENDER_WORKSPACE_BYTES"""
    return int(pixels) * 12


CONSISTENCY_BAD_PROJECTION, CONSISTENCY_EMPTY_MASK, CONSISTENCY_NO_CALIB = 1, 2, 4      # t3d.h t3d_detect_consistency: bits of `flags`
CONSISTENCY_CALIB_WIDTH = 20          # Rtilt (9), K (9), image W, image H


class DetectConsistencyArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('B', i32), ('N', i32), ('n_valid', i32), ('ld_xyz', i32), ('xyz', F), ('logits', F),
                ('corners', F), ('rot_angle', F), ('box2d', D), ('calib_index', I), ('calib', D), ('n_calib', i32), ('counts', I),
                ('reproj', D)]


class DetectFuseArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('n_groups', i32), ('metric', i32), ('group_offsets', I), ('members', I), ('keep', U8),
                ('suppressed_by', I), ('rank', I), ('label', F), ('corners', F), ('weight', F), ('vote_threshold', f32), ('max_group', i32),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64), ('label_out', F), ('corners_out', F), ('n_votes', I)]


def detect_fuse_workspace_bytes(n):
    """t3d.h T3D_DETECT_FUSE_WORKSPACE_BYTES"""
    return (n + 1) // 2 * 8 + n * 16


DETECT_ENSEMBLE_MAX_VIEWS = 8        # t3d.h T3D_DETECT_ENSEMBLE_MAX_VIEWS


class DetectEnsembleArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('V', i32), ('metric', i32), ('label', F * DETECT_ENSEMBLE_MAX_VIEWS),
                ('weight', F * DETECT_ENSEMBLE_MAX_VIEWS), ('flip_mask', C.c_uint32), ('vote_threshold', f32), ('rot_angle', F), ('corners0', F),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64), ('label_out', F), ('corners_out', F), ('agreement', F),
                ('min_iou', F), ('anchor', I), ('n_votes', I)]


def detect_ensemble_workspace_bytes(n, V):
    """t3d.h T3D_DETECT_ENSEMBLE_WORKSPACE_BYTES"""
    return (n * (V * (V - 1) // 2) + 1) // 2 * 8


NMS_SWEEP_MAX_THRESHOLDS = 16        # t3d.h T3D_NMS_SWEEP_MAX_THRESHOLDS
SWEEP_MAX_CONFIGS = 65536            # t3d.h T3D_SWEEP_MAX_CONFIGS


class DetectNmsSweepArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('n_groups', i32), ('metric', i32), ('corners', F), ('score', F), ('group_offsets', I),
                ('members', I), ('max_group', i32), ('n_thresholds', i32), ('thresholds', f32 * NMS_SWEEP_MAX_THRESHOLDS), ('M', i32),
                ('listed_stride', i32), ('keep_stride', i32), ('config_threshold', I), ('listed', U8), ('workspace', C.c_void_p),
                ('workspace_bytes', C.c_uint64), ('keep', U8), ('n_kept', I)]


def detect_nms_sweep_workspace_bytes(n, max_group, n_thresholds):
    """t3d.h T3D_DETECT_NMS_SWEEP_WORKSPACE_BYTES"""
    return (n + 1) // 2 * 8 + n * ((max_group + 63) // 64) * n_thresholds * 8


class SunrgbdSweepArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('M', i32), ('mask', U8), ('det_index', I), ('mask_stride', i32), ('workspace', C.c_void_p),
                ('workspace_bytes', C.c_uint64), ('ap', D), ('n_det', I), ('n_tp', I), ('n_fp', I)]


def sunrgbd_sweep_workspace_bytes(M, G):
    """t3d.h T3D_SUNRGBD_SWEEP_WORKSPACE_BYTES"""
    return M * G * 4 + 8


BOOTSTRAP_MAX_REPLICATES = 65536     # t3d.h T3D_BOOTSTRAP_MAX_REPLICATES


class BootstrapWeightsArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('seed', C.c_uint32), ('R', i32), ('n_images', i32), ('stride', i32), ('weights', I)]


class SunrgbdBootstrapArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('R', i32), ('weights', I), ('weight_stride', i32), ('det_col', I), ('gt_col', I),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64), ('ap', D), ('n_pos', L), ('n_tp', L), ('n_fp', L)]


def sunrgbd_bootstrap_workspace_bytes(P):
    """t3d.h T3D_SUNRGBD_BOOTSTRAP_WORKSPACE_BYTES"""
    return P * 4 + 8


def sunrgbd_eval_workspace_bytes(P, G):
    """t3d.h T3D_SUNRGBD_EVAL_WORKSPACE_BYTES"""
    return (P + G) * 92 + 8


def sunrgbd_diagnose_workspace_bytes(P, G, Go):
    """t3d.h T3D_SUNRGBD_DIAGNOSE_WORKSPACE_BYTES"""
    return Go * 88 + G * 4 + 8


def sunrgbd_locparts_workspace_bytes(P, G):
    """t3d.h T3D_SUNRGBD_LOCPARTS_WORKSPACE_BYTES"""
    return G * 20 + 8


def rescore_slices(n):
    """t3d.h T3D_RESCORE_SLICES"""
    return (n + RESCORE_SLICE - 1) // RESCORE_SLICE


def rescore_fit_workspace_bytes(n):
    """t3d.h T3D_RESCORE_FIT_WORKSPACE_BYTES"""
    return (128 + rescore_slices(n) * 368) * 8


# t3d.h T3D_SCENE_*
SCENE_MAX_PARTS, SCENE_MAX_OBJECTS, SCENE_BLOCK_PIXELS = 512, 64, 1024
SCENE_HIT_ROOM, SCENE_HIT_INVALID = -1, -2
SCENE_ROOM_COLOUR = 200.0
SCENE_SHADES = (0.70, 0.80, 0.60, 0.90, 0.50, 1.00)      # faces -x +x -y +y -z +z


class ScenePart(C.Structure):
    _fields_ = [('centre', C.c_double * 3), ('half', C.c_double * 3), ('cos_r', C.c_double), ('sin_r', C.c_double),
                ('colour', C.c_double * 3), ('owner', C.c_int32), ('reserved', C.c_int32)]


class SceneRaycastArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n_scenes', i32), ('H', i32), ('W', i32), ('stride', i32), ('seed', C.c_uint32),
                ('reserved', i32), ('rtilt', D), ('K', D), ('scene_id', I), ('room', D), ('part_offsets', I), ('parts', C.POINTER(ScenePart)),
                ('room_host', D), ('part_offsets_host', I), ('n_objects_host', I), ('noise_a', C.c_double), ('p_drop', C.c_double),
                ('max_range', C.c_double), ('min_cos2', C.c_double), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64),
                ('points_capacity', C.c_int64), ('hit', I), ('image', U8), ('points', D), ('point_pixel', I), ('scene_offsets', L),
                ('visible', I), ('vis_box', I)]


def scene_blocks(H, W):
    """t3d.h T3D_SCENE_BLOCKS"""
    return (H * W + SCENE_BLOCK_PIXELS - 1) // SCENE_BLOCK_PIXELS


def scene_workspace_bytes(S, H, W):
    """t3d.h T3D_SCENE_WORKSPACE_BYTES"""
    return S * scene_blocks(H, W) * 16


# t3d.h T3D_SCENE_FLOOR_* / T3D_FLOOR_* / T3D_DETECT_FLOOR_*
SCENE_FLOOR_MAX_BINS, SCENE_FLOOR_CHUNK, SCENE_FLOOR_BLOCKS = 1024, 4096, 64
FLOOR_NONE, FLOOR_LEVEL = 1, 2
DETECT_FLOOR_NO_FLOOR, DETECT_FLOOR_NOT_FINITE, DETECT_FLOOR_TOO_FAR, DETECT_FLOOR_INVERTED, DETECT_FLOOR_SNAPPED = 1, 2, 4, 8, 16


class SceneFloorArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n_scenes', i32), ('ld', i32), ('n_bins', i32), ('points', D), ('scene_offsets', L),
                ('z_lo', C.c_double), ('z_hi', C.c_double), ('bin', C.c_double), ('inv_bin', C.c_double), ('min_share', C.c_double),
                ('min_inliers', i32), ('reserved', i32), ('band', C.c_double), ('max_slope2', C.c_double), ('min_spread', C.c_double),
                ('min_det_ratio', C.c_double), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64), ('plane', D), ('counts', I),
                ('hist', I)]


def scene_floor_workspace_bytes(S):
    """t3d.h T3D_SCENE_FLOOR_WORKSPACE_BYTES"""
    return S * SCENE_FLOOR_BLOCKS * 80


class DetectFloorArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('n_scenes', i32), ('mode', i32), ('label', F), ('corners', F), ('scene_index', I),
                ('plane', D), ('counts', I), ('max_snap', C.c_double), ('reserved', i32), ('gap', D), ('flags', I), ('label_out', F),
                ('corners_out', F)]


# t3d.h T3D_RANGE_* / T3D_VIS_*
RANGE_EMPTY, RANGE_BLOCKS, RANGE_MAX_CELLS = 0x7F800000, 64, 1 << 24
RANGE_NO_CALIB, RANGE_BAD_GRID = 1, 2
VIS_MAX_OFFSETS = 17
VIS_NO_SCENE, VIS_NOT_FINITE, VIS_BEHIND, VIS_NO_RAYS, VIS_NO_EVIDENCE, VIS_SNAPPED = 1, 2, 4, 8, 16, 32
VIS_PROFILE = ('rays', 'unknown', 'front', 'inside', 'through', 'graze')          # the columns of a profile row
U32 = C.POINTER(C.c_uint32)


class SceneRangeArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n_scenes', i32), ('ld', i32), ('cell', i32), ('n_calib', i32), ('points', D), ('scene_offsets', L),
                ('calib', D), ('calib_index', I), ('grid_dims', I), ('grid_offsets', L), ('n_cells', C.c_int64), ('reserved', i32), ('range', U32),
                ('counts', I)]


class DetectVisibilityArgs(Sized):
    _fields_ = [('struct_size', C.c_uint32), ('n', i32), ('n_scenes', i32), ('mode', i32), ('K', i32), ('cell', i32), ('min_gain', i32),
                ('reserved', i32), ('label', F), ('corners', F), ('scene_index', I), ('calib', D), ('grid_dims', I), ('grid_offsets', L),
                ('range', U32), ('n_cells', C.c_int64), ('margin', C.c_double), ('min_chord', C.c_double),
                ('offsets', C.c_double * VIS_MAX_OFFSETS), ('profile', I), ('measures', D), ('choice', I), ('flags', I), ('label_out', F),
                ('corners_out', F)]


VP = C.c_void_p
# name -> argtypes.  Struct entry points take (const args*, stream).

class PoolBwdMidArgs(C.Structure):
    _fields_ = [('slab_base', F), ('grad_base', F), ('table_dev', C.POINTER(SlabDesc)), ('n_tensors', i32), ('max_numel', i32),
                ('sparse', PoolSparseRowsArgs)]


class SmallOpU(C.Union):
    _fields_ = [('bn_bwd', BnBwdFinalizeArgs), ('fc_bwd', FcBwdArgs), ('fc_dinput', FcDinputArgs), ('dy_colsum', DyColsumArgs),
                ('bn_fwd', BnFwdFinalizeArgs), ('fc_fwd', FcFwdArgs), ('mid', PoolBwdMidArgs)]


class SmallOp(C.Structure):
    _fields_ = [('kind', i32), ('depends', i32), ('u', SmallOpU)]


RIDER_MAX_OPS = 10            # t3d.h T3D_RIDER_MAX_OPS


class RiderSet(C.Structure):
    _fields_ = [('ops', SmallOp * RIDER_MAX_OPS), ('n_ops', i32), ('n_wg', i32), ('lds_bytes', i32), ('sync', C.POINTER(C.c_uint32))]


ENTRY_POINTS = {
    't3d_abi_version': [],
    't3d_gemm_arithmetic': [i32, i32, i32, i32, i32],
    't3d_source_hash': [C.c_char_p, C.c_int],
    't3d_pointmlp_fwd': [C.POINTER(PointMlpFwdArgs), VP],
    't3d_bn_fwd_finalize': [C.POINTER(BnFwdFinalizeArgs), VP],
    't3d_pool_finalize': [C.POINTER(PoolFinalizeArgs), VP],
    't3d_pointmlp_dgrad': [C.POINTER(PointMlpDgradArgs), VP],
    't3d_pointmlp_wgrad': [C.POINTER(PointMlpWgradArgs), VP],
    't3d_pointmlp_bwd': [C.POINTER(PointMlpDgradArgs), C.POINTER(PointMlpWgradArgs), VP],
    't3d_wgrad_plan': [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
    't3d_bwd_plan': [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)],
    't3d_weak_loss': [C.POINTER(WeakLossArgs), VP],
    't3d_small_pair': [C.POINTER(SmallOp), C.POINTER(SmallOp), VP],
    't3d_riders_plan': [C.POINTER(RiderSet)],
    't3d_run_riders': [C.POINTER(RiderSet), VP],
    't3d_pointmlp_fwd_r': [C.POINTER(PointMlpFwdArgs), C.POINTER(RiderSet), VP],
    't3d_pointmlp_wgrad_r': [C.POINTER(PointMlpWgradArgs), C.POINTER(RiderSet), VP],
    't3d_pointmlp_bwd_r': [C.POINTER(PointMlpDgradArgs), C.POINTER(PointMlpWgradArgs), C.POINTER(RiderSet), VP],
    't3d_pool_bwd_stage1_r': [C.POINTER(PointMlpGramArgs), C.POINTER(ActColsumArgs), C.POINTER(PoolBwdPrepArgs), C.POINTER(RiderSet), VP],
    't3d_pool_bwd_stage2_r': [C.POINTER(PoolWgradFinishArgs), C.POINTER(PointMlpDgradGramArgs), C.POINTER(RiderSet), VP],
    't3d_pointmlp_fwd_hosts_riders': [C.POINTER(PointMlpFwdArgs)],
    't3d_pointmlp_wgrad_hosts_riders': [C.POINTER(PointMlpWgradArgs)],
    't3d_pointmlp_bwd_hosts_riders': [C.POINTER(PointMlpDgradArgs), C.POINTER(PointMlpWgradArgs)],
    't3d_pool_bwd_stage1_hosts_riders': [C.POINTER(PointMlpGramArgs), C.POINTER(ActColsumArgs), C.POINTER(PoolBwdPrepArgs)],
    't3d_pool_bwd_stage2_hosts_riders': [C.POINTER(PoolWgradFinishArgs), C.POINTER(PointMlpDgradGramArgs)],
    't3d_gram_plan': [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)],
    't3d_bn_bwd_finalize': [C.POINTER(BnBwdFinalizeArgs), VP],
    't3d_dy_colsum': [C.POINTER(DyColsumArgs), VP],
    't3d_pool_bwd_prep': [C.POINTER(PoolBwdPrepArgs), VP],
    't3d_pool_sparse_rows': [C.POINTER(PoolSparseRowsArgs), VP],
    't3d_pointmlp_dgrad_gram': [C.POINTER(PointMlpDgradGramArgs), VP],
    't3d_pointmlp_gram': [C.POINTER(PointMlpGramArgs), VP],
    't3d_act_colsum': [C.POINTER(ActColsumArgs), VP],
    't3d_pool_wgrad_finish': [C.POINTER(PoolWgradFinishArgs), VP],
    't3d_batch_assemble': [C.POINTER(BatchAssembleArgs), VP],
    't3d_box_refine_step': [C.POINTER(BoxRefineStepArgs), VP],
    't3d_box_refine_step_bwd': [C.POINTER(BoxRefineStepBwdArgs), VP],
    't3d_boxpc_perturb': [C.POINTER(BoxPcPerturbArgs), VP],
    't3d_sample_equal_classes': [C.POINTER(SampleEqualClassesArgs), VP],
    't3d_box3d_iou': [C.POINTER(Box3dIouArgs), VP],
    't3d_box3d_iou_corners': [C.POINTER(Box3dIouCornersArgs), VP],
    't3d_box_head_iou': [C.POINTER(BoxHeadIouArgs), VP],
    't3d_box2d_feats': [C.POINTER(Box2dFeatsArgs), VP],
    't3d_pool_bwd_stage1': [C.POINTER(PointMlpGramArgs), C.POINTER(ActColsumArgs), C.POINTER(PoolBwdPrepArgs), VP],
    't3d_pool_bwd_mid': [F, F, C.POINTER(SlabDesc), i32, i32, C.POINTER(PoolSparseRowsArgs), VP],
    't3d_pool_bwd_stage2': [C.POINTER(PoolWgradFinishArgs), C.POINTER(PointMlpDgradGramArgs), VP],
    't3d_fc_fwd': [C.POINTER(FcFwdArgs), VP],
    't3d_fc_bwd': [C.POINTER(FcBwdArgs), VP],
    't3d_fc_dinput': [C.POINTER(FcDinputArgs), VP],
    't3d_seg_head': [C.POINTER(SegHeadArgs), VP],
    't3d_seg_finalize': [C.POINTER(SegFinalizeArgs), VP],
    't3d_act_dropout': [C.POINTER(ActDropoutArgs), VP],
    't3d_strong_loss': [C.POINTER(StrongLossArgs), VP],
    't3d_boxpc_rep': [C.POINTER(BoxPcRepArgs), VP],
    't3d_boxpc_rep_b': [C.POINTER(BoxPcRepBArgs), VP],
    't3d_boxpc_rep_bwd': [C.POINTER(BoxPcRepBwdArgs), VP],
    't3d_boxpc_loss': [C.POINTER(BoxPcLossArgs), VP],
    't3d_pointmlp_dgrad_narrow': [C.POINTER(DgradNarrowArgs), VP],
    't3d_semi_final_loss': [C.POINTER(SemiFinalLossArgs), VP],
    't3d_anchor_reg_bwd': [C.POINTER(AnchorRegBwdArgs), VP],
    't3d_reduce_slabs': [F, F, C.POINTER(SlabDesc), i32, i32, VP],
    't3d_schedule_step': [F, C.POINTER(Schedule), VP],
    't3d_reduce_slabs_adam': [F, F, C.POINTER(SlabDesc), i32, i32, F, F, F, C.POINTER(AdamRange), i32, i32, F, f32, f32, f32, f32, VP],
    't3d_step_head_takes': [C.POINTER(PointMlpFwdArgs)],
    't3d_step_head': [C.POINTER(PointMlpFwdArgs), F, VP, VP, C.c_int64, VP, i32, i32, F, C.POINTER(Schedule), VP],
    't3d_adam_tf_step': [F, F, F, F, C.c_int64, F, f32, f32, f32, f32, VP],
    't3d_momentum_step': [F, F, F, C.c_int64, F, f32, f32, VP],
    't3d_split_x3': [F, VP, C.c_int64, C.c_int64, VP],
    't3d_split_x3_frag': [F, VP, VP, C.c_int64, VP, i32, i32, VP],
    't3d_dropout_mask': [F, C.c_int64, f32, C.c_uint32, F, VP],
    't3d_cast_bf16': [F, VP, C.c_int64, VP],
    't3d_frustum_extract': [C.POINTER(FrustumExtractArgs), VP],
    't3d_sunrgbd_eval': [C.POINTER(SunrgbdEvalArgs), VP],
    't3d_sunrgbd_diagnose': [C.POINTER(SunrgbdEvalArgs), C.POINTER(SunrgbdDiagnoseArgs), VP],
    't3d_sunrgbd_locparts': [C.POINTER(SunrgbdEvalArgs), C.POINTER(SunrgbdDiagnoseArgs), C.POINTER(SunrgbdLocPartsArgs), VP],
    't3d_rescore_features': [C.POINTER(RescoreFeaturesArgs), VP],
    't3d_rescore_fit': [C.POINTER(RescoreFitArgs), VP],
    't3d_rescore_apply': [C.POINTER(RescoreApplyArgs), VP],
    't3d_scene_raycast': [C.POINTER(SceneRaycastArgs), VP],
    't3d_scene_floor': [C.POINTER(SceneFloorArgs), VP],
    't3d_detect_floor': [C.POINTER(DetectFloorArgs), VP],
    't3d_scene_range': [C.POINTER(SceneRangeArgs), VP],
    't3d_detect_visibility': [C.POINTER(DetectVisibilityArgs), VP],
    't3d_detect_decode': [C.POINTER(DetectDecodeArgs), VP],
    't3d_detect_nms': [C.POINTER(DetectNmsArgs), VP],
    't3d_render': [C.POINTER(RenderArgs), VP],
    't3d_detect_consistency': [C.POINTER(DetectConsistencyArgs), VP],
    't3d_detect_fuse': [C.POINTER(DetectFuseArgs), VP],
    't3d_detect_ensemble': [C.POINTER(DetectEnsembleArgs), VP],
    't3d_detect_nms_sweep': [C.POINTER(DetectNmsSweepArgs), VP],
    't3d_detect_soft_nms': [C.POINTER(DetectSoftNmsArgs), VP],
    't3d_sunrgbd_eval_sweep': [C.POINTER(SunrgbdEvalArgs), C.POINTER(SunrgbdSweepArgs), VP],
    't3d_bootstrap_weights': [C.POINTER(BootstrapWeightsArgs), VP],
    't3d_sunrgbd_eval_bootstrap': [C.POINTER(SunrgbdEvalArgs), C.POINTER(SunrgbdBootstrapArgs), VP],
    't3d_semi_sample': [C.POINTER(SemiSampleArgs), VP],
    't3d_label_subset': [C.POINTER(LabelSubsetArgs), VP],
}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libt3d.so')
ERRORS = {-1: 'T3D_ERR_ARG', -2: 'T3D_ERR_SHAPE', -3: 'T3D_ERR_LAUNCH'}


class T3DError(RuntimeError):
    pass


def source_hash_of(lib):
    """The source hash compiled into a loaded library (csrc/version.hip)."""
    buf = C.create_string_buffer(64)
    check(lib.t3d_source_hash(buf, 64), 't3d_source_hash')
    return buf.value.decode()


def load(path=None):
    """dlopen libt3d.so and bind every entry point of include/t3d.h; raises if anything is missing, and if the library was built
    from other sources than the ones lying next to it (T3D_ALLOW_STALE_LIB=1: experiments only)."""
    # torch bundles its own libamdhip64: import it FIRST so that libt3d.so binds to the same HIP runtime
    # instance that owns torch's streams and allocations (two runtimes in one process cannot share them).
    import torch  # noqa: F401
    variant = path or os.environ.get('T3D_LIB')                # T3D_LIB: an alternative build (tools/build_variant.sh) for same-box A/B
    path = variant or LIB_PATH
    if not os.path.exists(path):
        raise T3DError('HIP library %s not built: run `python -m transferable3d_amd.build` (no CPU fallback exists)' % path)
    lib = C.CDLL(path)
    for name, argtypes in ENTRY_POINTS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise T3DError('%s does not export %s' % (path, name))
        fn.argtypes = argtypes
        fn.restype = C.c_int
    if lib.t3d_abi_version() != ABI_VERSION:      # every library, the variants of the tools included
        raise T3DError('%s speaks ABI version %d, this host side version %d (include/t3d.h): rebuild it' % (path, lib.t3d_abi_version(), ABI_VERSION))
    from .build import CSRC, lib_source_hash
    if not variant and os.path.isdir(CSRC) and os.environ.get('T3D_ALLOW_STALE_LIB', '0') != '1':
        built, src = source_hash_of(lib), lib_source_hash()
        if built != src:
            raise T3DError('%s was built from other sources (library %s, csrc/ + include/t3d.h %s): run '
                           '`python -m transferable3d_amd.build`' % (path, built, src))
    return lib


def fptr(t):
    """float* of a tensor (None -> NULL)."""
    return C.cast(C.c_void_p(0 if t is None else t.data_ptr()), F)


def iptr(t):
    return C.cast(C.c_void_p(0 if t is None else t.data_ptr()), I)


def u8ptr(t):
    return C.cast(C.c_void_p(0 if t is None else t.data_ptr()), U8)


def dptr(t):
    return C.cast(C.c_void_p(0 if t is None else t.data_ptr()), D)


def grown(t, n, dtype, device, *width):
    """A wrapper's output or workspace of at least n rows [*width] of `dtype` on `device` (a workspace of 8-byte words: int64 rows): `t`
    where it holds that many already, else a new zeroed tensor of max(n, 1) rows.  The wrapper object keeps what this returns; such
    buffers are not the runtime's, because they are replaced as they grow."""
    import torch
    if t is not None and t.shape[0] >= n:
        return t
    return torch.zeros(max(n, 1), *width, dtype=dtype, device=device)


def check(rc, what):
    if rc != 0:
        raise T3DError('%s failed: %s' % (what, ERRORS.get(rc, rc)))
