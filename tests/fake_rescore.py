"""TEST INFRASTRUCTURE ONLY -- NumPy fp64 executable specification of t3d_rescore_features, t3d_rescore_fit and t3d_rescore_apply
(include/t3d.h, csrc/rescore.hip) on host pointers, so that transferable3d_amd/rescore.py and the flows behind it run end to end through
Runtime(device='cpu', lib=FakeRescoreLib()).  The fit is the entry point's algorithm: standardised columns, the start at the weighted
share of positives, damped Newton with the halving rule on the accepted loss, the convergence test on the gradient of the
weight-normalised objective, the same status bits.  What differs is the order of the sums (NumPy's pairwise sums over all rows, no
slices) and the Cholesky (LAPACK's): roundings, which tests/rescore_check.py bounds."""
import numpy as np

from fake_consistency import ConsistencySpec
from fake_detect import DetectDecodeSpec
from fake_ensemble import DetectEnsembleSpec
from fake_frustum import FakeFrustumLib
from fake_fuse import DetectFuseSpec
from fake_nms import DetectNmsSpec
from fake_render import RenderSpec
from fake_soft_nms import DetectSoftNmsSpec
from fake_sunrgbd_eval import FakeSunrgbdEvalLib
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

MAX_F, MAX_HALVINGS = abi.RESCORE_MAX_FEATURES, abi.RESCORE_MAX_HALVINGS
NO_ROWS, ONE_CLASS, CONSTANT_COLUMN, NOT_CONVERGED, NONFINITE = (abi.RESCORE_NO_ROWS, abi.RESCORE_ONE_CLASS, abi.RESCORE_CONSTANT_COLUMN,
                                                                 abi.RESCORE_NOT_CONVERGED, abi.RESCORE_NONFINITE)


def features(mask, prob=None, score=None, reproj=None, counts=None, view_iou=None):
    """The columns of t3d_rescore_features for the set bits of `mask`, in bit order -> [n, popcount] fp64."""
    cols = []
    with np.errstate(divide='ignore', invalid='ignore'):
        if mask & 1:
            q = np.asarray(prob, np.float32).astype(np.float64)
            q = np.where(q < 1e-6, 1e-6, q)
            q = np.where(q > 1.0 - 1e-6, 1.0 - 1e-6, q)
            cols.append(np.log(q / (1.0 - q)))
        if mask & 2:
            cols.append(np.asarray(score, np.float32).astype(np.float64))
        if mask & 4:
            cols.append(np.asarray(reproj, np.float64)[:, 4])
        if mask & (8 | 16 | 32):
            c = np.asarray(counts, np.int64)
            n_mask, n_box, n_both = c[:, 0], c[:, 1], c[:, 2]
            union = n_mask + n_box - n_both
            if mask & 8:
                cols.append(np.where(n_mask > 0, n_both.astype(np.float64) / np.maximum(n_mask, 1).astype(np.float64), 0.0))
            if mask & 16:
                cols.append(np.where(union > 0, n_both.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0))
            if mask & 32:
                cols.append(np.log1p(n_mask.astype(np.float64)))
        if mask & 64:
            cols.append(np.asarray(view_iou, np.float32).astype(np.float64))
    return np.stack(cols, 1)


def apply(coef, X):
    """t3d_rescore_apply: the intercept, then the products in column order, each rounded; 1 / (1 + exp(-z))."""
    coef, X = np.asarray(coef, np.float64), np.asarray(X, np.float64)
    F = len(coef) - 1
    z = np.full(len(X), coef[F])
    for j in range(F):
        z = z + coef[j] * X[:, j]
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-z))


def evaluate(w, Xs, y, r, lam):
    """At the point w (F coefficients, then the intercept) on the standardised rows that take part: (J, gradient, Hessian), all of
    the weight-normalised objective."""
    F = Xs.shape[1]
    A = np.concatenate([Xs, np.ones((len(Xs), 1))], 1)
    W = r.sum()
    z = A @ w
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(-np.abs(z))
        q = 1.0 / (1.0 + e)
        p = np.where(z >= 0, q, e * q)
        J = np.sum(r * (np.maximum(z, 0.0) - y * z + np.log1p(e))) / W + 0.5 * lam * np.sum(w[:F] ** 2)
        ridge = np.concatenate([np.full(F, lam), [0.0]])
        g = A.T @ (r * (p - y)) / W + ridge * w
        H = (A * (r * (e * q * q))[:, None]).T @ A / W + np.diag(ridge)
    return J, g, H


def fit(X, y, r, lam, max_iter=30, gtol=1e-9):
    """t3d_rescore_fit -> dict(coef, coef_std, mean, scale, loss [max_iter], n_iter, status, n_rows, n_pos) and, for the tests,
    hessian (of the standardised problem at the last accepted point, or None) and n_eval (the evaluations that ran)."""
    X, y, r = np.asarray(X, np.float64), (np.asarray(y) != 0).astype(np.float64), np.asarray(r, np.float64)
    n, F = X.shape
    max_iter, gtol = max_iter or 30, gtol or 1e-9
    out = dict(coef=np.zeros(F + 1), coef_std=np.zeros(F + 1), mean=np.zeros(F), scale=np.ones(F), loss=np.full(max_iter, np.nan), n_iter=0,
               status=0, n_rows=0, n_pos=0, hessian=None, n_eval=0)
    live = r > 0
    X, y, r = X[live], y[live], r[live]
    out['n_rows'], out['n_pos'] = int(live.sum()), int(y.sum())
    if not (np.isfinite(X).all() and np.isfinite(r).all()):
        out['status'] = NONFINITE
        return out
    W, Wy = r.sum(), (r * y).sum()
    if not W > 0:
        out['status'] = NO_ROWS
        return out
    mean = (r[:, None] * X).sum(0) / W
    sd = np.sqrt((r[:, None] * (X - mean) ** 2).sum(0) / W)
    same = X.min(0) == X.max(0)
    constant = same | ~(sd > 0)
    mean = np.where(same, X.min(0), mean)
    scale = np.where(constant, 1.0, sd)
    out['mean'], out['scale'] = mean, scale
    status = CONSTANT_COLUMN if constant.any() else 0
    inv = 1.0 / scale

    def raw(w):
        c = w[:F] * inv
        b = w[F]
        for j in range(F):
            b = b - c[j] * mean[j]
        return np.concatenate([c, [b]])
    if out['n_pos'] in (0, out['n_rows']):
        q = (Wy + 0.5) / (W + 1.0)
        w = np.concatenate([np.zeros(F), [np.log(q / (1.0 - q))]])
        out.update(status=status | ONE_CLASS, coef_std=w, coef=raw(w))
        return out
    Xs = (X - mean) * inv
    trial = np.concatenate([np.zeros(F), [np.log(Wy / (W - Wy))]])
    accepted, step, J_acc, halvings, n_acc, converged = trial, np.zeros(F + 1), None, 0, 0, False
    for _ in range(max_iter):
        J, g, H = evaluate(trial, Xs, y, r, lam)
        out['n_eval'] += 1
        if (n_acc == 0 and J == J) or (n_acc > 0 and J <= J_acc):
            accepted, J_acc, halvings = trial, J, 0
            out['loss'][n_acc] = J
            n_acc += 1
            out['hessian'] = H
            if np.all(np.abs(g) <= gtol):
                converged = True
                break
            try:
                L = np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                break
            step = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            trial = accepted + step
        elif n_acc == 0:
            break
        else:
            halvings += 1
            if halvings > MAX_HALVINGS:
                break
            step = 0.5 * step
            trial = accepted + step
    out.update(status=status | (0 if converged else NOT_CONVERGED), n_iter=n_acc, coef_std=accepted, coef=raw(accepted))
    return out


def standard_errors(X, r, coef):
    """The asymptotic standard errors of a fitted raw model (F coefficients, then the intercept): the square roots of the diagonal of
    the inverse of A^T diag(r p (1 - p)) A, A = [X, 1]."""
    X, r = np.asarray(X, np.float64), np.asarray(r, np.float64)
    A = np.concatenate([X, np.ones((len(X), 1))], 1)
    p = apply(coef, X)
    return np.sqrt(np.diag(np.linalg.inv((A * (r * p * (1 - p))[:, None]).T @ A)))


def popcount(m):
    return bin(int(m)).count('1')


class RescoreSpec:
    def t3d_rescore_features(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        m = p.feature_mask
        if not p.X or m == 0 or m >> len(abi.RESCORE_FEATURES):
            return -1
        if p.n < 0 or p.ld < popcount(m):
            return -2
        if (m & 1 and not p.prob) or (m & 2 and not p.score) or (m & 4 and not p.reproj) or (m & 56 and not p.counts) or (m & 64 and not p.view_iou):
            return -1
        n = p.n
        if n == 0:
            return 0
        cols = features(m, arr(p.prob, n), arr(p.score, n), arr(p.reproj, n, 5), arr(p.counts, n, 4), arr(p.view_iou, n))
        arr(p.X, n, p.ld)[:, :cols.shape[1]] = cols
        return 0

    def t3d_rescore_fit(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if p.reserved != 0:
            return -1
        n, F = p.n, p.F
        if n < 0 or F < 1 or F > MAX_F or p.ld < F:
            return -2
        if not (p.lambda_ > 0 and np.isfinite(p.lambda_)) or not p.gtol >= 0 or p.max_iter < 0 or p.max_iter > 1000:
            return -1
        if not all([p.coef, p.coef_std, p.mean, p.scale, p.loss, p.n_iter, p.status, p.n_rows, p.n_pos]):
            return -1
        if n > 0 and not (p.X and p.y and p.r):
            return -1
        if not p.workspace or p.workspace % 8 or p.workspace_bytes < abi.rescore_fit_workspace_bytes(n):
            return -1
        max_iter = p.max_iter or 30
        X = arr(p.X, n, p.ld)[:, :F] if n else np.zeros((0, F))
        o = fit(X, arr(p.y, n) if n else np.zeros(0), arr(p.r, n) if n else np.zeros(0), p.lambda_, max_iter, p.gtol)
        if o['status'] & NONFINITE:
            o['mean'], o['scale'] = np.full(F, np.nan), np.full(F, np.nan)      # (whatever the sums gave: not to be used)
        arr(p.coef, F + 1)[:], arr(p.coef_std, F + 1)[:], arr(p.mean, F)[:], arr(p.scale, F)[:] = o['coef'], o['coef_std'], o['mean'], o['scale']
        arr(p.loss, max_iter)[:] = o['loss']
        p.n_iter[0], p.status[0], p.n_rows[0], p.n_pos[0] = o['n_iter'], o['status'], o['n_rows'], o['n_pos']
        return 0

    def t3d_rescore_apply(self, a, stream):
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if p.reserved != 0 or not p.X or not p.coef or not p.out:
            return -1
        if p.n < 0 or p.n_valid < 0 or p.n_valid > p.n or p.F < 1 or p.F > MAX_F or p.ld < p.F:
            return -2
        nv = p.n_valid
        if nv == 0:
            return 0
        v = apply(arr(p.coef, p.F + 1), arr(p.X, p.n, p.ld)[:nv, :p.F])
        arr(p.out, p.n)[:nv] = v
        if p.out32:
            arr(p.out32, p.n)[:nv] = v.astype(np.float32)
        return 0


class FakeRescoreLib(RescoreSpec, DetectSoftNmsSpec, DetectEnsembleSpec, ConsistencySpec, RenderSpec, DetectFuseSpec, DetectNmsSpec, DetectDecodeSpec,
                     FakeFrustumLib, FakeSunrgbdEvalLib):
    """Everything `detect` and `autolabel` call behind the decode, plus the evaluation the fit takes its targets from."""
