"""TEST INFRASTRUCTURE ONLY -- the executable specification of t3d_bootstrap_weights and t3d_sunrgbd_eval_bootstrap (include/t3d.h,
csrc/sunrgbd_bootstrap.hip).  The weights are the header's hash in Python integers.  The evaluation of a replicate is, ON PURPOSE, not
weighted: `expand` builds the resampled data set literally -- copy k of an image gets a fresh id, its boxes are copied, the copies of a
detection are adjacent in file order -- and the existing evaluation (FakeSunrgbdEvalLib.t3d_sunrgbd_eval, or any library's) runs on it.
That the weighted curve of the kernel equals this is then a tested statement, not an assumption the two sides share.  BootstrapSpec is
the mix-in that puts both behind the ctypes structs on host pointers, so that bootstrap.Weights, evaluate_sunrgbd.bootstrap_class and the
command lines run end to end through Runtime(device='cpu', lib=...)."""
import numpy as np

from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi, evaluate_sunrgbd as ES

MAX_REPLICATES = 1 << 16
M64 = (1 << 64) - 1


def mix_u32(x):
    """The finaliser of csrc/data.hip / csrc/frustum.hip on a Python integer (64-bit wrapping)."""
    x &= M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return (x >> 16) & 0xffffffff


def draw(seed, r, d, n_images):
    """The column of draw d of replicate r (t3d.h, t3d_bootstrap_weights)."""
    key = ((((seed << 32) | r) * 0x9E3779B97F4A7C15) + (d + 1) * 0xD6E8FEB86659FD93) & M64
    return (mix_u32(key) * n_images) >> 32


def weights(seed, R, n_images, stride=None):
    """-> int32 [R, stride]: how often each column is drawn; the columns from n_images on are 0."""
    w = np.zeros((R, n_images if stride is None else stride), np.int32)
    for r in range(R):
        for d in range(n_images):
            w[r, draw(seed, r, d, n_images)] += 1
    return w


def column_weights(cols, row):
    """The weight of every column of `cols` in the row; 0 for a column outside [0, len(row))."""
    cols = np.asarray(cols, np.int64).reshape(-1)
    ok = (cols >= 0) & (cols < len(row))
    w = np.zeros(len(cols), np.int64)
    w[ok] = np.asarray(row, np.int64)[cols[ok]]
    return w


def expand(det, gt, det_col, gt_col, row):
    """The resampled data set of one replicate, literally: -> (det', gt').  Copy k of the image with id X becomes the image with a fresh id
    (one per distinct (X, k), in ascending order of (X, k), so distinct copies never share an id); box g is copied weight(gt_col[g])
    times, detection i weight(det_col[i]) times, the copies adjacent, everything else in its order."""
    wd, wg = column_weights(det_col, row), column_weights(gt_col, row)
    di, gi = np.repeat(np.arange(len(wd)), wd), np.repeat(np.arange(len(wg)), wg)
    dk = np.concatenate([np.arange(w) for w in wd] + [np.zeros(0, np.int64)]).astype(np.int64)
    gk = np.concatenate([np.arange(w) for w in wg] + [np.zeros(0, np.int64)]).astype(np.int64)
    dimg, gimg = np.asarray(det['image'], np.int64)[di], np.asarray(gt['image'], np.int64)[gi]
    pairs = sorted(set(zip(dimg.tolist(), dk.tolist())) | set(zip(gimg.tolist(), gk.tolist())))
    fresh = {p: n for n, p in enumerate(pairs)}
    out_d = {k: np.asarray(v)[di] for k, v in det.items() if k != 'classname'}
    out_g = {k: np.asarray(v)[gi] for k, v in gt.items() if k != 'classname'}
    out_d['image'] = np.asarray([fresh[p] for p in zip(dimg.tolist(), dk.tolist())], np.int32)
    out_g['image'] = np.asarray([fresh[p] for p in zip(gimg.tolist(), gk.tolist())], np.int32)
    return out_d, out_g


def literal(evaluate, det, gt, det_col, gt_col, matrix):
    """evaluate(det', gt') -> the arrays of one evaluation ('ap', 'is_tp', 'is_fp').  -> {'ap' float64 [R], 'n_pos', 'n_tp', 'n_fp'
    int64 [R]}: per row of the matrix the evaluation of the literally resampled data set."""
    R = len(matrix)
    out = {'ap': np.zeros(R), 'n_pos': np.zeros(R, np.int64), 'n_tp': np.zeros(R, np.int64), 'n_fp': np.zeros(R, np.int64)}
    for r in range(R):
        d, g = expand(det, gt, det_col, gt_col, matrix[r])
        e = evaluate(d, g)
        out['ap'][r], out['n_pos'][r] = e['ap'][0], len(g['image'])
        out['n_tp'][r], out['n_fp'][r] = int((e['is_tp'] != 0).sum()), int((e['is_fp'] != 0).sum())
    return out


class BootstrapSpec:
    """Mix-in: t3d_bootstrap_weights and t3d_sunrgbd_eval_bootstrap for a specification library that has t3d_sunrgbd_eval."""

    def t3d_bootstrap_weights(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if not p.weights:
            return -1
        if not 1 <= p.R <= MAX_REPLICATES or p.n_images < 1:
            return -2
        if p.stride < p.n_images:
            return -1
        arr(p.weights, p.R, p.stride)[:] = weights(p.seed, p.R, p.n_images, p.stride)
        return 0

    def t3d_sunrgbd_eval_bootstrap(self, a, b, stream):
        from transferable3d_amd.engine import Runtime
        try:
            p, q = _struct(a), _struct(b)
        except AbiSizeError:
            return abi.ERR_ABI
        if not (q.weights and q.ap and q.n_pos and q.n_tp and q.n_fp) or p.gt_difficult:
            return -1
        if p.P < 0 or p.G < 0 or not 1 <= q.R <= MAX_REPLICATES or not 1 <= q.weight_stride <= 1 << 30:
            return -2
        if (p.P > 0 and not q.det_col) or (p.G > 0 and not q.gt_col):
            return -1
        if p.P > 0 and (not q.workspace or q.workspace_bytes < abi.sunrgbd_bootstrap_workspace_bytes(p.P) or q.workspace % 8):
            return -1
        e = self.t3d_sunrgbd_eval(a, stream)
        if e != 0:
            return e
        P, G = p.P, p.G
        box = lambda c, k, n: np.array(arr(c, n, k)) if n else np.zeros((0, k))
        det = {'centroid': box(p.det_centroid, 3, P), 'basis': box(p.det_basis, 9, P).reshape(P, 3, 3), 'coeffs': box(p.det_coeffs, 3, P),
               'confidence': np.array(arr(p.det_confidence, P)) if P else np.zeros(0), 'image': np.array(arr(p.det_image, P)) if P else np.zeros(0, np.int32)}
        gt = {'centroid': box(p.gt_centroid, 3, G), 'basis': box(p.gt_basis, 9, G).reshape(G, 3, 3), 'coeffs': box(p.gt_coeffs, 3, G),
              'image': np.array(arr(p.gt_image, G)) if G else np.zeros(0, np.int32)}
        det_col = np.array(arr(q.det_col, P)) if P else np.zeros(0, np.int32)
        gt_col = np.array(arr(q.gt_col, G)) if G else np.zeros(0, np.int32)
        rt = Runtime(device='cpu', lib=self)
        out = literal(lambda d, g: ES._eval_call(d, g, None, p.threshold, rt), det, gt, det_col, gt_col, np.array(arr(q.weights, q.R, q.weight_stride)))
        for name, v in out.items():
            arr(getattr(q, name), q.R)[:] = v
        return 0
