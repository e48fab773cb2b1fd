"""What the three training drivers (train_semisup: stage a, train_boxpc: stage b, train_semisup_adv: stage c) have in common: the
shared command-line flags, the feed of a synthetic batch into the semisup placeholders, the per-frustum detection / label boxes of the
two eval_one_epochs, and the epoch skeleton (`run_epochs`).  A driver keeps what is its own: its graph, what it fetches and
accumulates, its epoch lines, its evaluation.  Where the drivers differ in ways that show in logs, checkpoints or synchronisation
points, the difference is kept and marked `as found` at the place that makes it."""
import os
import time

import numpy as np

from transferable3d_amd import api
from transferable3d_amd.constants import MEAN_DIMS_ARR, NUM_HEADING_BIN, class2type


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def add_point_arguments(cfg):
    """The flags every driver -- the inference driver test_semisup included -- reads the point layout, the seed and the element type from."""
    cfg.add_argument('--no_rgb', action='store_true', help='Only use XYZ for training')
    cfg.add_argument('--num_channels', type=int, default=None, help='override point channels (reference: 6, or 3 with --no_rgb)')
    cfg.add_argument('--seed', type=int, default=0)
    cfg.add_argument('--dtype', default='f32', choices=['f32', 'bf16'],
                     help='element type of the per-point layer tensors and GEMM operands (bf16: BASELINE configs[4]; weights, statistics, heads, losses and Adam stay fp32)')


def add_training_arguments(cfg, log_dir, steps_per_epoch, model, train_data_choices=None):
    """The flags of all three training drivers (the reference's train_*.py:28-48 and this project's additions); the arguments are the
    defaults that differ between them."""
    cfg.add_argument('--train_data', type=str, default='synthetic', choices=train_data_choices)
    cfg.add_argument('--gpu', type=int, default=0, help='GPU to use [default: GPU 0]')
    cfg.add_argument('--model', default=model, help='Model name [default: %s]' % model)
    cfg.add_argument('--log_dir', default=log_dir, help='Log dir [default: %s]' % log_dir)
    cfg.add_argument('--num_point', type=int, default=2048, help='Point Number [default: 2048]')
    cfg.add_argument('--max_epoch', type=int, default=31, help='Epoch to run [default: 31]')
    cfg.add_argument('--batch_size', type=int, default=32, help='Batch Size during training [default: 32]')
    cfg.add_argument('--learning_rate', type=float, default=0.001, help='Initial learning rate [default: 0.001]')
    cfg.add_argument('--momentum', type=float, default=0.9)
    cfg.add_argument('--optimizer', default='adam', help='adam or momentum [default: adam]')
    cfg.add_argument('--decay_step', type=int, default=800000, help='Decay step for lr decay [default: 800000]')
    cfg.add_argument('--decay_rate', type=float, default=0.5, help='Decay rate for lr decay [default: 0.5]')
    cfg.add_argument('--use_one_hot', action='store_true', help='Use one hot vector during training')
    cfg.add_argument('--restore_model_path', default=None, help='Restore model path e.g. log/model_epoch_0.ckpt or .npz')
    cfg.add_argument('--ckpt_format', default='npz', choices=['npz', 'tf'], help='tf: TensorFlow Saver bundle')
    # additions
    cfg.add_argument('--synthetic', action='store_true', help='synthetic frustums (the only data source available)')
    cfg.add_argument('--steps_per_epoch', type=int, default=steps_per_epoch,
                     help='steps of an epoch [default: %s]' % (steps_per_epoch or 'one pass over the data set, len / (batch_size * replicas) as in '
                                                               'the reference; 100 for --synthetic batches'))
    cfg.add_argument('--device_data', type=int, default=0, metavar='F',
                     help='keep a synthetic data set of F ragged frustums in HBM and make every batch on the device (t3d_batch_assemble: '
                          'resample / centre-view rotation / flip / shift / labels; stage b: the perturbed-box samples, t3d_boxpc_perturb; '
                          'stage c under ALTERNATE_BATCH: weak / strong batches on alternate steps)')
    cfg.add_argument('--eval_file', default=None, help='held-out frustum file of the reference for eval_one_epoch (with --frustum_file / --device_data)')
    cfg.add_argument('--frustum_file', default=None, help='train from a frustum file of the reference (frustums/*.zip.pickle) held in HBM')
    cfg.add_argument('--eval_batches', type=int, default=0, help='held-out synthetic batches evaluated after every epoch (eval_one_epoch)')
    add_point_arguments(cfg)


def finish_flags(FLAGS):
    FLAGS.NUM_CHANNELS = FLAGS.num_channels if FLAGS.num_channels else (3 if FLAGS.no_rgb else 6)
    return FLAGS


# ---- feeds and boxes -----------------------------------------------------------------------------------------------------------------
def semi_feed(pls, batch, is_data_2D=None):
    """A synthetic.make_batch dict -> the placeholders of semisup_v1_sunrgbd.placeholder_inputs (bg_pc, img, R0_rect and P are never
    fed).  `is_data_2D`: instead of the batch's own flags (evaluation: every frustum with its 3-D label)."""
    pc_pl, _, _, one_hot_vec_pl, y_seg_pl, y_centers_pl, y_orient_cls_pl, y_orient_reg_pl, y_dims_cls_pl, y_dims_reg_pl, _, _, \
        Rtilt_pl, K_pl, rot_frust_pl, box2D_pl, img_dim_pl, is_data_2D_pl = pls
    return {pc_pl: batch['pc'], one_hot_vec_pl: batch['one_hot_vec'], y_seg_pl: batch['y_seg'], y_centers_pl: batch['y_center'],
            y_orient_cls_pl: batch['y_orient_cls'], y_orient_reg_pl: batch['y_orient_reg'], y_dims_cls_pl: batch['y_dims_cls'],
            y_dims_reg_pl: batch['y_dims_reg'], is_data_2D_pl: batch['is_data_2D'] if is_data_2D is None else is_data_2D,
            # camera side of the weak losses (their default weights are non-zero: models/config.py:112-113)
            Rtilt_pl: batch['Rtilt'], K_pl: batch['K'], rot_frust_pl: batch['rot_frust'], box2D_pl: batch['box2D'],
            img_dim_pl: batch['img_dim']}


LABEL_FIELDS = ('y_center', 'y_orient_cls', 'y_orient_reg', 'y_dims_cls', 'y_dims_reg', 'one_hot_vec')


def _class_names(one_hot_vec):
    return [class2type[int(c)] for c in np.argmax(one_hot_vec, 1)]


def boxes_from_heads(lab, logits, heads):
    """[(class name, corners [8, 3], score)] per frustum of a batch (main_batch + evaluate_predictions, train_semisup.py:459-466): the box
    of the arg-max heading bin and size cluster with their residuals, in the frustum's centre view; the class is the label's.
    heads = (center, heading_scores, heading_residuals, size_scores, size_residuals); lab: the LABEL_FIELDS as arrays."""
    from transferable3d_amd.eval_det import get_3d_box
    from transferable3d_amd.test_semisup import detection_scores
    cen, hs, hr, ss, sr = heads
    hc, sc, score = np.argmax(hs, 1), np.argmax(ss, 1), detection_scores(logits, hs, ss)
    return [(cls, get_3d_box(MEAN_DIMS_ARR[sc[k]] + sr[k, sc[k]], hc[k] * (2 * np.pi / NUM_HEADING_BIN) + hr[k, hc[k]], cen[k]), float(score[k]))
            for k, cls in enumerate(_class_names(lab['one_hot_vec']))]


def boxes_from_labels(lab):
    """[(class name, corners [8, 3])] per frustum: the label boxes the detections of boxes_from_heads are scored against."""
    from transferable3d_amd.eval_det import get_3d_box
    return [(cls, get_3d_box(MEAN_DIMS_ARR[int(lab['y_dims_cls'][k])] + lab['y_dims_reg'][k],
                             int(lab['y_orient_cls'][k]) * (2 * np.pi / NUM_HEADING_BIN) + float(lab['y_orient_reg'][k]), lab['y_center'][k]))
            for k, cls in enumerate(_class_names(lab['one_hot_vec']))]


# ---- the epoch skeleton --------------------------------------------------------------------------------------------------------------
def start(FLAGS, rt, log):
    """(world, rank, process group, log): joins the data-parallel group (one process per GPU) and makes log_dir.  Rank 0
    logs and checkpoints: on every other rank `log` is a no-op, so no caller guards a log call by rank."""
    world, rank, pg = api.init_data_parallel(rt, FLAGS.gpu)
    os.makedirs(FLAGS.log_dir, exist_ok=True)
    return world, rank, pg, (log if rank == 0 else (lambda *a, **k: None))


def host_seed(FLAGS, step, world, rank):
    """Seed of the synthetic host batch of a training step (every replica its own); an evaluation batch i uses eval_seed.  Both as found,
    like the seeds the drivers keep: the device data set `seed + 17 * rank`, use_device_dataset `seed * 7919 + rank`, dropout `1234 + rank`."""
    return FLAGS.seed * 1000003 + step * world + rank


def eval_seed(FLAGS, i):
    return FLAGS.seed * 1000003 + 900000 + i


def run_epochs(FLAGS, sess, saver, world, rank, log, ds, is_training_pl, fetches, train_op, fetch_on, host_feed, begin_epoch, record,
               epoch_lines, evaluate, iters=1, optimizer_scopes=None):
    """FLAGS.max_epoch epochs of FLAGS.steps_per_epoch * iters steps each; returns the final state dict.
    Device path (`ds`, a data set resident in HBM): one shuffle, then nothing is fed; `fetches` are fetched -- a D2H sync -- on the steps
    `fetch_on(it, n_steps)` picks, `train_op` runs alone on the others.  Host path (ds None): `host_feed(seed, it, step)` makes the
    feed of every step and every step is fetched.  A fetched step goes to `record(out)`; `begin_epoch()` resets what record
    accumulates.  After the steps: `epoch_lines(epoch, n_fetched, n_steps, t0)`, then `evaluate(epoch)` on rank 0, then, every fifth
    epoch on rank 0, the checkpoint (train_semisup.py:316-318) -- never of weights a timed-out rider barrier may have corrupted."""
    g, step = sess.g, 0
    for epoch in range(FLAGS.max_epoch):
        t0 = time.time()
        begin_epoch()
        n_steps, n_fetched = FLAGS.steps_per_epoch * iters, 0
        if ds is not None:
            ds.shuffle(FLAGS.seed * 1000003 + epoch)      # train_semisup.py:343 (the same permutation on every replica)
            for it in range(n_steps):
                if fetch_on(it, n_steps):
                    record(sess.run(fetches))
                    n_fetched += 1
                else:
                    sess.run([train_op])
                step += 1
        else:
            for it in range(n_steps):
                feed = host_feed(host_seed(FLAGS, step, world, rank), it, step)
                feed[is_training_pl] = True
                record(sess.run(fetches, feed_dict=feed))
                n_fetched += 1
                step += 1
        epoch_lines(epoch, n_fetched, n_steps, t0)
        if rank == 0:
            evaluate(epoch)
            if epoch % 5 == 0:
                sess.check_riders()
                log('Model saved in file: %s' % saver.save(FLAGS.log_dir, epoch, g, FLAGS.ckpt_format, optimizer_scopes=optimizer_scopes))
    sess.check_riders()
    final = g.vars.state_dict()
    api.finish_data_parallel(world)
    return final
