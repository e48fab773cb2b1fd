"""The percentile bootstrap over images for the official SUN-RGBD AP (include/t3d.h: t3d_bootstrap_weights, t3d_sunrgbd_eval_bootstrap;
csrc/sunrgbd_bootstrap.hip).

Every comparison of two AP numbers -- with and without --nms_fuse, the rows of a --sweep -- needs to know how far the number moves when
the validation images are redrawn.  `Weights` is the device matrix of R redraws (how often each image of the list occurs in each),
made once per run and shared by all classes and by both sides of a comparison, which makes the comparison paired: each image is its own
control.  evaluate_sunrgbd.bootstrap_class turns it into R APs of one class; `summary` and `paired` (host, NumPy) turn those into
means, standard errors, percentile intervals and, for a difference, the share of replicates in which it is <= 0.
"""
import ctypes as C

import numpy as np
import torch

from . import abi

MIN_REPLICATES, MAX_REPLICATES = 100, abi.BOOTSTRAP_MAX_REPLICATES      # what the command lines take; the entry points take R >= 1


class Weights:
    """weights[R, n_images] int32 on the runtime's device: row r counts how often each image is drawn when n_images are drawn with
    replacement (the counter-based hash of t3d.h, keyed by seed, r and the draw).  Equal (n_images, R, seed) give equal bytes."""

    def __init__(self, rt, n_images, R, seed=0):
        n_images, R, seed = int(n_images), int(R), int(seed)
        if not 1 <= R <= MAX_REPLICATES:
            raise ValueError('R lies in [1, %d]' % MAX_REPLICATES)
        if n_images < 1:
            raise ValueError('a bootstrap needs at least one image')
        if not 0 <= seed < 2 ** 32:
            raise ValueError('the seed is an unsigned 32-bit number')
        self.rt, self.n_images, self.R, self.seed = rt, n_images, R, seed
        self.matrix = torch.empty(R, n_images, dtype=torch.int32, device=rt.device)      # every element is written
        a = abi.BootstrapWeightsArgs(seed, R, n_images, n_images, abi.iptr(self.matrix))
        abi.check(rt.lib.t3d_bootstrap_weights(C.byref(a), rt.stream()), 't3d_bootstrap_weights')

    @classmethod
    def of(cls, rt, matrix, seed=None):
        """A given matrix (int32 [R, columns]; NumPy, uploaded, or a tensor on the runtime's device) in place of drawn weights."""
        self = cls.__new__(cls)
        if not torch.is_tensor(matrix):
            matrix = torch.from_numpy(np.ascontiguousarray(matrix, np.int32)).to(rt.device)
        if matrix.dtype != torch.int32 or matrix.dim() != 2 or not 1 <= matrix.shape[0] <= MAX_REPLICATES or matrix.shape[1] < 1:
            raise ValueError('weights is int32 [R, columns] with 1 <= R <= %d and at least one column' % MAX_REPLICATES)
        if matrix.shape[1] > 1 and matrix.stride(1) != 1:
            raise ValueError('the rows of the weight matrix are contiguous')
        self.rt, self.n_images, self.R, self.seed, self.matrix = rt, int(matrix.shape[1]), int(matrix.shape[0]), seed, matrix
        return self

    @property
    def stride(self):
        return int(self.matrix.stride(0)) if self.R > 1 else self.n_images

    def numpy(self):
        return self.matrix.cpu().numpy().copy()


def _interval(v, level):
    lo, hi = np.percentile(v, [50.0 * (1.0 - level), 50.0 * (1.0 + level)])
    return [float(lo), float(hi)]


def _describe(v, level):
    v = np.asarray(v, np.float64).reshape(-1)
    lo, hi = _interval(v, level)
    return {'mean': float(np.mean(v)), 'se': float(np.std(v, ddof=1)) if len(v) > 1 else 0.0, 'lo': lo, 'hi': hi}


def _check_level(level):
    if not 0.0 < float(level) < 1.0:
        raise ValueError('the level of an interval lies strictly between 0 and 1')
    return float(level)


def mean_over_classes(ap_by_class):
    """[R]: per replicate the mean over the classes (in the dictionary's order), as `evaluate` forms its mean AP."""
    ap = np.ascontiguousarray(np.stack([np.asarray(v, np.float64).reshape(-1) for v in ap_by_class.values()], 1))
    return np.mean(ap, axis=1)


def summary(ap_by_class, level=0.95):
    """{class: replicate APs [R]} -> {'level', 'R', 'classes': {class: {'mean', 'se', 'lo', 'hi'}}, 'mean_ap': the same of the mean over
    classes, taken per replicate}.  se: the standard deviation of the replicates (ddof 1); [lo, hi]: the percentile interval, the
    (1 - level) / 2 and (1 + level) / 2 quantiles with NumPy's linear interpolation."""
    level = _check_level(level)
    if not ap_by_class:
        raise ValueError('no class')
    R = {len(np.asarray(v).reshape(-1)) for v in ap_by_class.values()}
    if len(R) != 1:
        raise ValueError('the classes have different numbers of replicates')
    return {'level': level, 'R': R.pop(), 'classes': {c: _describe(v, level) for c, v in ap_by_class.items()},
            'mean_ap': _describe(mean_over_classes(ap_by_class), level)}


def _describe_difference(d, level):
    out = _describe(d, level)
    out['p_le0'] = float(np.mean(np.asarray(d) <= 0.0))
    return out


def paired(a, b, level=0.95):
    """`summary` of b - a per replicate, for two sets of replicate APs made with the SAME weights ({class: [R]} with equal classes), plus
    'p_le0' per entry: the share of replicates with difference <= 0."""
    level = _check_level(level)
    if list(a) != list(b):
        raise ValueError('the two sides hold different classes: %s, %s' % (list(a), list(b)))
    d = {c: np.asarray(b[c], np.float64).reshape(-1) - np.asarray(a[c], np.float64).reshape(-1) for c in a}
    return {'level': level, 'R': len(next(iter(d.values()))), 'classes': {c: _describe_difference(v, level) for c, v in d.items()},
            'mean_ap': _describe_difference(mean_over_classes(b) - mean_over_classes(a), level)}


def paired_vector(a, b, level=0.95):
    """`paired` for two vectors of replicate values (e.g. the mean AP of two sweep rows)."""
    return _describe_difference(np.asarray(b, np.float64).reshape(-1) - np.asarray(a, np.float64).reshape(-1), _check_level(level))


def interval_text(s, level, R, num2str):
    """'[lo, hi] (95 %, se s, R replicates)' for one entry of `summary`: values x 100 in the format of the AP lines (num2str)."""
    return '[%s, %s] (%g %%, se %s, %d replicates)' % (num2str(s['lo'] * 100.0), num2str(s['hi'] * 100.0), round(100.0 * level, 10),
                                                      num2str(s['se'] * 100.0), R)


def signed(x):
    """+1.32 / −0.41 (U+2212) / +0.00: a difference x 100 with two decimals."""
    t = '%.2f' % abs(x)
    return ('−' if x < 0 and float(t) != 0.0 else '+') + t


def difference_text(s):
    """'+1.32 [−0.41, +3.02], p(≤0) 0.07' for one entry of `paired` (values x 100)."""
    return '%s [%s, %s], p(≤0) %.2f' % (signed(100.0 * s['mean']), signed(100.0 * s['lo']), signed(100.0 * s['hi']), s['p_le0'])


def add_arguments(p):
    """--bootstrap and its three options, for evaluate_sunrgbd's parser and for detect's."""
    p.add_argument('--bootstrap', type=int, default=None, metavar='R',
                   help='percentile bootstrap over the images: R redraws of the image list (%d..%d), an interval behind every AP line' % (MIN_REPLICATES, MAX_REPLICATES))
    p.add_argument('--bootstrap_seed', type=int, default=None, help='--bootstrap: the seed of the redraws (default 0)')
    p.add_argument('--bootstrap_level', type=float, default=None, help='--bootstrap: the level of the intervals (default 0.95)')
    p.add_argument('--bootstrap_json', default=None, help="--bootstrap: write every class's replicate APs and the summaries to this file")


def options(p, FLAGS):
    """The `bootstrap` dictionary of `evaluate` from parsed flags (None without --bootstrap); a parser error where they contradict."""
    if FLAGS.bootstrap is None:
        if FLAGS.bootstrap_seed is not None or FLAGS.bootstrap_level is not None or FLAGS.bootstrap_json is not None:
            p.error('--bootstrap_seed / --bootstrap_level / --bootstrap_json need --bootstrap')
        return None
    if not MIN_REPLICATES <= FLAGS.bootstrap <= MAX_REPLICATES:
        p.error('--bootstrap takes %d to %d replicates' % (MIN_REPLICATES, MAX_REPLICATES))
    if getattr(FLAGS, 'diagnose', False):
        p.error('--diagnose and --bootstrap exclude each other: a diagnosis of the replicates is not defined')
    seed = 0 if FLAGS.bootstrap_seed is None else FLAGS.bootstrap_seed
    level = 0.95 if FLAGS.bootstrap_level is None else FLAGS.bootstrap_level
    if not 0 <= seed < 2 ** 32:
        p.error('--bootstrap_seed is an unsigned 32-bit number')
    if not 0.0 < level < 1.0:
        p.error('--bootstrap_level lies strictly between 0 and 1')
    return {'R': FLAGS.bootstrap, 'seed': seed, 'level': level, 'json': FLAGS.bootstrap_json}
