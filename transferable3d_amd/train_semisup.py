#!/usr/bin/env python3
"""Stage-a training driver (SEMI_MODEL A) with the reference's command line
(sunrgbd/sunrgbd_detection/train_semisup.py: flags 28-48, graph build 199-260, epoch loop 305-318, train_one_epoch
320-436).  Differences, all forced by the environment and documented in DESIGN.md:
  * `--synthetic` batches (transferable3d_amd/synthetic.py) replace the SUN-RGBD frustum pickles, which are not
    available; `--train_data` is therefore optional.
  * one process per GPU: launch with `python -m torch.distributed.run --nproc-per-node N ... train_semisup.py` for
    data-parallel training (gradient all-reduce on RCCL); `--gpu` selects the device in the single-process case.
  * checkpoints are `.npz` state dicts keyed by the reference's TF variable names or, with
    `--ckpt_format tf`, TensorFlow Saver bundles (`model_epoch_<n>.ckpt.index/.data-*`, tf_checkpoint.py); `--restore_model_path`
    takes either.

Example (README.md:58-67 recipe a, synthetic data):
  python -m transferable3d_amd.train_semisup --SEMI_MODEL A --WEAK_WEIGHT_REPROJECTION 0 --WEAK_WEIGHT_SURFACE 0 \
      --num_point 1024 --no_rgb_channels 4 --max_epoch 1 --steps_per_epoch 100
"""
import argparse
import os
import sys
import time

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transferable3d_amd import api, tf_util, semisup_v1_sunrgbd as MODEL       # noqa: E402
from transferable3d_amd.config import make_parser                        # noqa: E402
from transferable3d_amd.synthetic import make_batch                      # noqa: E402
from transferable3d_amd.tf_checkpoint import Saver, restore_model   # noqa: E402
from transferable3d_amd.train_common import (LABEL_FIELDS, add_training_arguments, boxes_from_heads, boxes_from_labels, eval_seed,      # noqa: E402
                                             finish_flags, run_epochs, semi_feed, start)


def build_flags(argv=None):
    cfg = make_parser()
    add_training_arguments(cfg, log_dir='log', steps_per_epoch=None, model='semisup_v1_sunrgbd',
                           train_data_choices=['train_mini', 'train_aug5x', 'trainval_aug5x', 'synthetic'])
    add_label_subset_arguments(cfg)
    cfg.add_argument('--use_mini', action='store_true')
    cfg.add_argument('--no_aug', action='store_true')
    cfg.add_argument('--init_model_path', default=None)
    cfg.add_argument('--weak_loss_summaries', action='store_true',
                     help='evaluate the weak reprojection / surface losses also when both of their weights are 0, for the reference\'s '
                          'Weak_Loss/... summaries (semisup_v1_sunrgbd.py:270-293; logged per epoch).  Off by default since round 6: the two '
                          'launches cost 22 us of a 1.2 ms step (+1.9 %%) and change nothing that is trained -- SURVEY Appendix E item 4 '
                          'sanctions skipping zero-weight terms; with a non-zero weight they are always evaluated')
    cfg.add_argument('--no_weak_loss_summaries', action='store_true', help='(accepted for round-5 command lines: the default now)')
    given = sampling_method_on_command_line(cfg, argv)
    FLAGS = finish_flags(StageAFlags(**vars(cfg.parse_special_args(argv))))
    FLAGS.SEMI_SAMPLING_METHOD_GIVEN = given
    FLAGS.WEAK_LOSS_SUMMARIES = bool(FLAGS.weak_loss_summaries) and not FLAGS.no_weak_loss_summaries
    label_subset_flags(FLAGS)          # (a probability outside [-1, 1] raises here)
    return FLAGS


def add_label_subset_arguments(cfg):
    """train_semisup.py:35-36 / train_semisup_adv.py:29-30: how much of the 3-D supervision the 3-D-label list keeps."""
    cfg.add_argument('--train_data3D_keep_prob', type=float, default=1,
                     help='every frustum of the classes with 3-D labels stays in the 3-D-label list with this probability')
    cfg.add_argument('--add3D_for_classes2D_prob', type=float, default=-1,
                     help='a frustum that did not enter the 3-D-label list that way (any class) is added to it with this probability')
    cfg.add_argument('--label_subset_seed', type=int, default=20,
                     help="seed of the serial np.random walk that decides the subset [the reference's fixed 20]")


def label_subset_flags(FLAGS):
    """(keep_prob, add_prob, seed, asked): `asked` when either probability differs from its default."""
    from transferable3d_amd.dataset import _checked_prob
    keep = _checked_prob('train_data3D_keep_prob', getattr(FLAGS, 'train_data3D_keep_prob', 1))
    add = _checked_prob('add3D_for_classes2D_prob', getattr(FLAGS, 'add3D_for_classes2D_prob', -1))
    return keep, add, int(getattr(FLAGS, 'label_subset_seed', 20)), (keep != 1.0 or add != -1.0)


def label_subset_member(FLAGS, ds):
    """uint8 flags [F] of the 3-D-label list under --train_data3D_keep_prob / --add3D_for_classes2D_prob (the reference's serial walk
    replayed on the host, dataset.reference_label_subset), or None when both flags have their defaults."""
    from transferable3d_amd.constants import type2class
    from transferable3d_amd.dataset import reference_label_subset
    keep, add, seed, asked = label_subset_flags(FLAGS)
    if not asked:
        return None
    names = getattr(ds, 'class_names', None)                 # a frustum file; a synthetic set has class ids only
    classes3d = list(FLAGS.SUNRGBD_SEMI_TRAIN_CLS)
    if names is None:
        names, classes3d = ds.cls.cpu().numpy().tolist(), [type2class[t] for t in classes3d]
    return reference_label_subset(names, classes3d, keep, add, seed)


SEMI_SAMPLING_METHODS = ('BATCH', 'ALTERNATE_BATCH', 'MIXED_BATCH')
_PARSER_DEFAULT_METHOD = 'ALTERNATE_BATCH'       # config.py, as in the reference


def sampling_method_on_command_line(parser, argv=None):
    """Does the command line (`argv` None: sys.argv) set SEMI_SAMPLING_METHOD?  Asked of the parser itself -- a parse with no default
    for the flag -- so that every spelling argparse accepts counts (`--SEMI_SAMPLING_METHOD=X`, an unambiguous abbreviation)."""
    default = parser.get_default('SEMI_SAMPLING_METHOD')
    parser.set_defaults(SEMI_SAMPLING_METHOD=None)
    try:
        return parser.parse_args(argv).SEMI_SAMPLING_METHOD is not None
    finally:
        parser.set_defaults(SEMI_SAMPLING_METHOD=default)


class StageAFlags(argparse.Namespace):
    """The namespace build_flags returns: assigning SEMI_SAMPLING_METHOD afterwards (a caller that passes FLAGS to train) counts as
    asking for that method, the parser's default value included."""

    def __setattr__(self, name, value):
        if name == 'SEMI_SAMPLING_METHOD':
            object.__setattr__(self, 'SEMI_SAMPLING_METHOD_GIVEN', True)
        object.__setattr__(self, name, value)


def requested_sampling_method(FLAGS):
    """(method, asked): the SEMI_SAMPLING_METHOD the user asked for, or (None, False).  Stage a has always walked the combined data
    set (BATCH) whatever the parser's default (ALTERNATE_BATCH, the reference's) said, and existing command lines rely on it -- so the
    flag counts only when it was given: on the command line (build_flags asks the parser), by a caller that assigns it in the FLAGS
    build_flags returned (StageAFlags notes it) or sets FLAGS.SEMI_SAMPLING_METHOD_GIVEN, or -- a namespace from elsewhere -- by a value
    other than the parser's default.  A method that is asked for is honoured or refused, never replaced."""
    method = getattr(FLAGS, 'SEMI_SAMPLING_METHOD', _PARSER_DEFAULT_METHOD)
    asked = bool(getattr(FLAGS, 'SEMI_SAMPLING_METHOD_GIVEN', False)) or method != _PARSER_DEFAULT_METHOD
    if not asked:
        return None, False
    if method not in SEMI_SAMPLING_METHODS:
        raise ValueError('unknown SEMI_SAMPLING_METHOD %r (known: %s)' % (method, ', '.join(SEMI_SAMPLING_METHODS)))
    return method, True


def classes_2d(FLAGS, test_cls=None):
    """train_semisup.py:97 / train_semisup_adv.py:105: the classes of the 2-D-label list."""
    test_cls = list(FLAGS.SUNRGBD_SEMI_TEST_CLS if test_cls is None else test_cls)
    if FLAGS.SEMI_USE_LABELS2D_OF_CLASSES3D:
        return sorted(set(list(FLAGS.SUNRGBD_SEMI_TRAIN_CLS) + test_cls))
    return test_cls


def eval_one_epoch(sess, ops, FLAGS, epoch, log, source=None):
    """train_semisup.py:436-545 on held-out synthetic frustums: the SAME graph with is_training fed False (moving batch-norm
    statistics, no dropout, no parameter or EMA update) -- loss, segmentation accuracy / class accuracy / IoU, box IoU."""
    pls, is_training_pl, semi_loss, n_correct, end_points = ops
    B, N, C = FLAGS.batch_size, FLAGS.num_point, FLAGS.NUM_CHANNELS
    from transferable3d_amd.eval_det import eval_det, get_ap_info
    det_all, gt_all = {}, {}
    log('---- EPOCH %03d EVALUATION ----' % epoch)
    loss_sum = iou2 = iou3 = 0.0
    seen, correct = np.zeros(2), np.zeros(2)
    shape_ious = []
    for i in range(FLAGS.eval_batches):
        if source is not None:                               # batch assembled on the device: nothing but the mode is fed
            lab = source.load(i)
            feed = {is_training_pl: False}
        else:
            b = make_batch(B, N, C, seed=eval_seed(FLAGS, i))
            lab = b['y_seg']
            feed = semi_feed(pls, b, is_data_2D=np.zeros(B, np.int32))
            feed[is_training_pl] = False
        heads = [end_points[k] for k in ('center', 'heading_scores', 'heading_residuals', 'size_scores', 'size_residuals')]
        loss_val, logits, i2, i3, *heads = sess.run(
            [semi_loss, end_points_logits(end_points, sess), end_points['iou2ds'], end_points['iou3ds']] + heads, feed_dict=feed)
        pred = np.argmax(logits, 2)
        # detections of this batch and their label boxes; every frustum is its own image
        lab_box = {k: getattr(sess.g.inputs, k).cpu().numpy() for k in LABEL_FIELDS}
        for k, (det, gt) in enumerate(zip(boxes_from_heads(lab_box, logits, heads), boxes_from_labels(lab_box))):
            det_all[i * B + k], gt_all[i * B + k] = [det], [gt]
        loss_sum += float(loss_val)
        iou2, iou3 = iou2 + float(np.sum(i2)), iou3 + float(np.sum(i3))
        for l in range(2):
            seen[l] += np.sum(lab == l)
            correct[l] += np.sum((pred == l) & (lab == l))
        for k in range(B):                                   # per-frustum part IoU; an absent part that is not predicted counts 1
            shape_ious.append([1.0 if not (np.any(lab[k] == l) or np.any(pred[k] == l)) else
                               np.sum((lab[k] == l) & (pred[k] == l)) / float(np.sum((lab[k] == l) | (pred[k] == l))) for l in range(2)])
    n = float(FLAGS.eval_batches)
    log('eval mean loss: %f' % (loss_sum / n))
    log('eval accuracy: %f' % (correct.sum() / seen.sum()))
    log('eval avg class acc: %f' % np.mean(correct / np.maximum(seen, 1)))
    log('eval mIoU: %f' % np.mean(shape_ious))
    log('eval box IoU (ground/3D)     : %f / %f' % (iou2 / (n * B), iou3 / (n * B)))
    _, _, ap = eval_det(det_all, gt_all, 0.25, rt=sess.g.rt)
    log(get_ap_info(ap, float(np.mean(list(ap.values())))))
    log(ap_by_label_kind(ap, FLAGS))
    return loss_sum / n


def ap_by_label_kind(ap, FLAGS):
    """Mean AP over the classes trained with 3-D labels and over the classes with 2-D labels only (the reference evaluates the
    latter: TEST_DATASET holds FLAGS.TEST_CLS, train_semisup.py:113-117)."""
    weak = [ap[k] for k in ap if k in FLAGS.SUNRGBD_SEMI_TEST_CLS]
    strong = [ap[k] for k in ap if k not in FLAGS.SUNRGBD_SEMI_TEST_CLS]
    m = lambda v: 100.0 * float(np.mean(v)) if v else float('nan')
    return '    Mean AP, classes with 3-D labels: %.1f   classes with 2-D labels only: %.1f' % (m(strong), m(weak))


def end_points_logits(end_points, sess):
    g = sess.g
    return api.Tensor(g, g.assembly.seg.logits, (g.engine.B, g.engine.rpf, 2), 'logits')


def train(FLAGS, rt=None, log=print):
    method, asked = requested_sampling_method(FLAGS)      # (an unknown method raises before anything is built)
    world, rank, pg, log = start(FLAGS, rt, log)
    B, N, C = FLAGS.batch_size, FLAGS.num_point, FLAGS.NUM_CHANNELS
    log(FLAGS.config_str)                 # as found: stage a alone logs its configuration first
    iters = 1
    with api.Graph(rt=rt, seed=FLAGS.seed, inline_dropout=True, dtype=FLAGS.dtype).as_default() as g:
        pls = MODEL.placeholder_inputs(B, N, C)
        is_training_pl = api.is_training_placeholder()                     # train_semisup.py:210
        norm_box2D = tf_util.tf_normalize_2D_bboxes(pls[15], pls[16])       # train_semisup.py:240 (dropped unless USE_NORMALIZED_BOX2D_AS_FEATS)
        pred, end_points = MODEL.get_semi_model(pls[0], pls[1], pls[2], pls[3], is_training_pl, use_one_hot=FLAGS.use_one_hot,
                                                norm_box2D=norm_box2D, bn_decay=None, c=FLAGS)
        semi_loss = MODEL.get_semi_loss(pred, tuple(pls[4:]), end_points, c=FLAGS)
        optimizer = api.make_optimizer(FLAGS, world_size=world)      # train_semisup.py:226-231 (--optimizer adam | momentum)
        train_op = optimizer.minimize(semi_loss)
        sess = api.Session(process_group=pg, dropout_seed=1234 + rank)
        saver = Saver(max_to_keep=5)      # train_semisup.py:259
        if FLAGS.restore_model_path:
            restore_model(g, FLAGS.restore_model_path)
        n_correct = api.Tensor(g, g.assembly.seg.n_correct, (1,), 'n_correct')
        from transferable3d_amd.dataset import open_training_set
        ds = open_training_set(g.rt, FLAGS, C, classes=list(FLAGS.SUNRGBD_SEMI_TRAIN_CLS) + list(FLAGS.SUNRGBD_SEMI_TEST_CLS),
                               seed=FLAGS.seed + 17 * rank)
        if ds is not None:
            # SEMI_SAMPLING_METHOD (train_semisup.py:97-110, 340-380).  BATCH over the combined data set: frustums of the classes that
            # have 2-D labels only (SUNRGBD_SEMI_TEST_CLS) run through the net with is_data_2D = 1 -- no strong loss, their points
            # still enter the batch statistics.  Known deviation: the method is taken from the flag only when it was asked for
            # (requested_sampling_method); otherwise stage a runs BATCH, as it always has, and says so.
            from transferable3d_amd.constants import type2class
            ids = lambda names: [type2class[t] for t in names]
            run = method if asked else 'BATCH'
            if not asked:
                log('SEMI_SAMPLING_METHOD not given: stage a runs BATCH (the parsed default %s is not applied; pass '
                    '--SEMI_SAMPLING_METHOD to choose)' % getattr(FLAGS, 'SEMI_SAMPLING_METHOD', _PARSER_DEFAULT_METHOD))
            member3d = label_subset_member(FLAGS, ds)
            if run == 'BATCH' and not FLAGS.SEMI_USE_LABELS2D_OF_CLASSES3D and member3d is None:
                # every frustum is in exactly one list: a per-frustum flag on the one epoch permutation
                ds.mark_2d_classes(ids(FLAGS.SUNRGBD_SEMI_TEST_CLS))
                g.use_device_dataset(ds, seed=FLAGS.seed * 7919 + rank)
                len2d = int(ds.is_2D.sum())
                lengths = (len2d, ds.F - len2d)
            else:
                # t3d_semi_sample in front of the assembly: the 3-D-label list of TRAIN_CLS and the 2-D-label list (TEST_CLS, and
                # TRAIN_CLS once more as zero-loss 2-D samples under SEMI_USE_LABELS2D_OF_CLASSES3D); BATCH walks len3D + len2D entries
                # (a label subset -- --train_data3D_keep_prob / --add3D_for_classes2D_prob -- takes this path under every method: the
                # per-frustum flag cannot leave a frustum of a 3-D class out of the 3-D list)
                ds.semi_lists(ids(FLAGS.SUNRGBD_SEMI_TRAIN_CLS), ids(classes_2d(FLAGS)), member3d=member3d)
                lengths = (len(ds.semi[1]['host']), len(ds.semi[0]['host']))
                g.use_device_dataset(ds, seed=FLAGS.seed * 7919 + rank, semi_sampling=run,
                                     equal_class_prob=float(FLAGS.SEMI_SAMPLE_EQUAL_CLASS_WITH_PROB))
                iters = 2 if run == 'ALTERNATE_BATCH' else 1      # train_semisup.py:340: a 2-D and a 3-D batch per batch index
                log('SEMI_SAMPLING_METHOD %s on the device: %d frustums with 3-D labels, %d with 2-D labels' % (
                    run, len(ds.semi[0]['host']), len(ds.semi[1]['host'])))
            api.assert_ranks_agree(pg, world, lengths, 'the label subset (2D, 3D)')
            log('Length of Train Dataset: (2D: %d, 3D: %d)' % lengths)       # train_semisup.py:104
            # an epoch = ONE pass (train_semisup.py:330-349: num_batches = len(TRAIN_DATASET) / BATCH_SIZE); data parallel: every
            # replica walks its own slice of the common epoch permutation, so the replicas see disjoint frustums
            n = ds.partition(rank, world, B, FLAGS.steps_per_epoch)
            if FLAGS.steps_per_epoch and n < FLAGS.steps_per_epoch:
                log('--steps_per_epoch %d exceeds one pass over the data set: %d steps per epoch' % (FLAGS.steps_per_epoch, n))
            FLAGS.steps_per_epoch = n      # as found: stage a always partitions on the device path, whatever the sampling method
        elif not FLAGS.steps_per_epoch:
            FLAGS.steps_per_epoch = 100
        # tf.summary.scalar('Weak_Loss/reprojection_loss' | 'Weak_Loss/surface_loss') of get_semi_loss_backbone: batch means, logged
        # per epoch (evaluated at zero weight too: --weak_loss_summaries)
        weak_t = [end_points[k] for k in ('reproj_loss', 'surface_loss') if k in end_points]
        acc = argparse.Namespace(loss_sum=0.0)
        eval_source = None

        def begin_epoch():
            acc.loss_sum = acc.correct = 0.0
            acc.iou2_sum = acc.iou3_sum = 0.0                 # 'Strong Box IoU (ground/3D)' of train_semisup.py:414-431
            acc.weak_sum = np.zeros(len(weak_t))

        def record(out):
            loss_val, nc, i2, i3, _, *wk = out
            acc.weak_sum = acc.weak_sum + np.array([float(np.mean(v)) for v in wk])
            acc.loss_sum += float(loss_val)
            acc.correct += float(nc[0])
            acc.iou2_sum, acc.iou3_sum = acc.iou2_sum + float(np.sum(i2)), acc.iou3_sum + float(np.sum(i3))

        def epoch_lines(epoch, n_fetched, n_steps, t0):
            log('**** EPOCH %03d ****  mean loss: %f  accuracy: %f  (%.1f frustums/s%s)' % (
                epoch, acc.loss_sum / n_fetched, acc.correct / (n_fetched * B * N), n_steps * B * world / (time.time() - t0),
                ', batches assembled on the device' if ds is not None else ' incl. host batch synthesis'))
            log('Strong Box IoU (ground/3D): %f / %f' % (acc.iou2_sum / (n_fetched * B), acc.iou3_sum / (n_fetched * B)))
            if ds is not None:      # as found: the returned loss is the mean over the fetched steps, scaled to the epoch and divided again
                acc.loss_sum = acc.loss_sum / n_fetched * FLAGS.steps_per_epoch
            if n_fetched and len(weak_t) == 2:
                log('Weak_Loss/reprojection_loss: %f  Weak_Loss/surface_loss: %f  (weights %g / %g)' % (
                    acc.weak_sum[0] / n_fetched, acc.weak_sum[1] / n_fetched, FLAGS.WEAK_WEIGHT_REPROJECTION, FLAGS.WEAK_WEIGHT_SURFACE))

        def evaluate(epoch):
            nonlocal eval_source
            if FLAGS.eval_batches > 0 or FLAGS.eval_file:
                if ds is not None and eval_source is None:      # as found: opened at the first evaluation, not before training
                    from transferable3d_amd.dataset import open_eval_source
                    eval_source = open_eval_source(g, FLAGS, classes=list(FLAGS.SUNRGBD_SEMI_TEST_CLS))   # TEST_DATASET, train_semisup.py:113
                eval_one_epoch(sess, (pls, is_training_pl, semi_loss, n_correct, end_points), FLAGS, epoch, log, eval_source)

        final = run_epochs(
            FLAGS, sess, saver, world, rank, log, ds, is_training_pl, iters=iters, train_op=train_op,
            fetches=[semi_loss, n_correct, end_points['iou2ds'], end_points['iou3ds'], train_op] + weak_t,
            # as found: every 10th step, and the last batch index (both of its steps under ALTERNATE_BATCH)
            fetch_on=lambda it, n_steps: it % 10 == 9 or it >= n_steps - iters,
            host_feed=lambda seed, it, step: semi_feed(pls, make_batch(B, N, C, seed=seed)),
            begin_epoch=begin_epoch, record=record, epoch_lines=epoch_lines, evaluate=evaluate)
    return final, acc.loss_sum / max(FLAGS.steps_per_epoch, 1)


if __name__ == '__main__':
    train(build_flags())
