"""Shared cases and checkers of the rescoring entry points (t3d_rescore_features / _fit / _apply): tests/test_rescore_cpu.py runs them
through the NumPy specification (tests/fake_rescore.py), tests/test_rescore_gpu.py through libt3d.so on the MI355X.

The bounds, and where each comes from:
  features   the columns without a transcendental (score, reproj_iou, mask_in_box, seg_box_iou, view_iou) bit for bit; logit_prob and
             log_mask within 2 ulps (log / log1p of two libraries, each within 1 ulp of the true value).
  apply      relative 2^-50 = 8 u (include/t3d.h: 4 u from the two exp, 2 u per rounded operation behind it).
  gradient   at the coefficients returned with status 0 the gradient recomputed here has |g|_inf <= 2 gtol (the recomputation's own
             rounding is ~1e-16 per term: seven orders below gtol = 1e-9).
  loss       the accepted losses never increase: exact.
  coef_std   MEASURED: the largest |difference| between the device and the specification over the well-conditioned cases (condition
             number of the standardised Hessian below 1e4, asserted per case) was taken on the MI355X; the bound is 8 x that, the
             project's convention (tests/test_sunrgbd_locparts_gpu.py).  The collinear case and the shapes too small for their F stay
             out of it: they are held by the gradient, and their `apply` outputs by the bound that follows from it --
             |dp| <= 1/4 max_i |a_i|_2 |dw|_2 and |dw|_2 <= (|g_a|_2 + |g_b|_2) / eig_min(H), both gradients <= 2 gtol per entry.
"""
import ctypes as C
import os

import numpy as np
import torch

import fake_rescore as FR
from transferable3d_amd import abi
from transferable3d_amd import rescore as RS

SLICE = abi.RESCORE_SLICE
GTOL = 1e-9
N_LIST = (1, 2, 63, 64, 65, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5)
F_LIST = (1, 3, 7, 15)
LAM = 1e-2                    # of the shape grid
COND_MAX = 1e4
# largest |coef_std(device) - coef_std(specification)| over the well-conditioned cases, measured on the MI355X (docs/EXPERIMENTS.md)
MEASURED_WORST = 4.514e-9      # n 65, F 1: one side stopped an iterate earlier (both within gtol); where both stop at the same iterate 4.8e-15 at worst
COEF_BOUND = 1e-9 if MEASURED_WORST is None else 8.0 * MEASURED_WORST
APPLY_REL = 2.0 ** -50


def well_conditioned(n, F):
    """The shapes whose coefficients are compared: enough rows per coefficient for classes that overlap (below that a random set is
    separable and the ridge alone holds the Hessian)."""
    return n >= 16 * (F + 1)


def dev(rt, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)


def padded(X, ld, fill=np.nan):
    """X in a [n, ld] buffer whose padding columns hold NaN: nothing may read them."""
    out = np.full((X.shape[0], ld), fill)
    out[:, :X.shape[1]] = X
    return out


def make_case(n, F, seed, weights='mixed', spread=1.0):
    """n rows from a known model: columns of different offsets and spreads, coefficients small enough for the classes to overlap.
    weights: 'ones', or 'mixed' -- a third zeros, a third ones, a third fractions in (0, 2)."""
    rng = np.random.RandomState(seed)
    offset, width = rng.uniform(-3, 3, F), rng.uniform(0.2, 4.0, F)
    Z = rng.randn(n, F)
    X = Z * width + offset
    w = rng.uniform(-1, 1, F) * spread / np.sqrt(F)
    b = rng.uniform(-0.5, 0.5)
    y = (rng.uniform(size=n) < 1 / (1 + np.exp(-(Z @ w + b)))).astype(np.uint8)
    if weights == 'ones':
        r = np.ones(n)
    else:
        kind = rng.randint(0, 3, n)
        r = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, rng.uniform(0.05, 2.0, n)))
        if n <= 2:
            r[:] = 1.0 if n == 1 else np.array([0.5, 1.5])
    return X, y, r


def call_fit(rt, X, y, r, lam, max_iter=30, gtol=0.0, ld=None, keep=None):
    """t3d_rescore_fit through `rt` on host arrays -> dict of host outputs (as fake_rescore.fit, without the Hessian) and 'raw': every
    output buffer's bytes."""
    n, F = X.shape
    ld = F + 3 if ld is None else ld
    d = lambda a: dev(rt, a)
    bufs = dict(X=d(padded(X, ld)) if n else None, y=d(np.asarray(y, np.uint8)) if n else None, r=d(np.asarray(r, np.float64)) if n else None,
                ws=rt.zeros(abi.rescore_fit_workspace_bytes(n) // 8, dtype=torch.float64))
    iters = max_iter or 30
    o = dict(coef=rt.full((F + 1,), 7.0, dtype=torch.float64), coef_std=rt.full((F + 1,), 7.0, dtype=torch.float64),
             mean=rt.full((F,), 7.0, dtype=torch.float64), scale=rt.full((F,), 7.0, dtype=torch.float64),
             loss=rt.full((iters,), 7.0, dtype=torch.float64), n_iter=rt.full((1,), -5, dtype=torch.int32),
             status=rt.full((1,), -5, dtype=torch.int32), n_rows=rt.full((1,), -5, dtype=torch.int64), n_pos=rt.full((1,), -5, dtype=torch.int64))
    a = abi.RescoreFitArgs(n, F, ld, max_iter, 0, abi.dptr(bufs['X']), abi.u8ptr(bufs['y']), abi.dptr(bufs['r']), lam, gtol,
                           C.c_void_p(bufs['ws'].data_ptr()), bufs['ws'].numel() * 8, abi.dptr(o['coef']), abi.dptr(o['coef_std']),
                           abi.dptr(o['mean']), abi.dptr(o['scale']), abi.dptr(o['loss']), abi.iptr(o['n_iter']),
                           C.cast(C.c_void_p(o['status'].data_ptr()), C.POINTER(C.c_uint32)),
                           C.cast(C.c_void_p(o['n_rows'].data_ptr()), abi.L), C.cast(C.c_void_p(o['n_pos'].data_ptr()), abi.L))
    rc = rt.lib.t3d_rescore_fit(C.byref(a), rt.stream())
    assert rc == 0, rc
    host = {k: v.cpu().numpy().copy() for k, v in o.items()}
    out = {k: (host[k] if k in ('coef', 'coef_std', 'mean', 'scale', 'loss') else int(host[k][0])) for k in host}
    out['status'] &= 0xffffffff
    out['raw'] = b''.join(host[k].tobytes() for k in sorted(host))
    if keep is not None:
        keep.update(bufs, **o)
    return out


def call_apply(rt, coef, X, n_valid=None, ld=None, want32=True):
    n, F = X.shape
    ld = F + 2 if ld is None else ld
    Xd, cd = dev(rt, padded(X, ld)), dev(rt, np.asarray(coef, np.float64))
    out, out32 = rt.full((n,), -3.0, dtype=torch.float64), rt.full((n,), -3.0)
    a = abi.RescoreApplyArgs(n, n if n_valid is None else n_valid, F, ld, 0, abi.dptr(Xd), abi.dptr(cd), abi.dptr(out), abi.fptr(out32 if want32 else None))
    rc = rt.lib.t3d_rescore_apply(C.byref(a), rt.stream())
    assert rc == 0, rc
    return out.cpu().numpy(), out32.cpu().numpy()


def ulps(a, b):
    """|a - b| in units of the spacing of b."""
    return np.abs(a - b) / np.spacing(np.abs(b))


def gradient(fit, X, y, r, lam):
    """The gradient of the weight-normalised objective at the returned standardised coefficients, with the returned mean and scale."""
    live = r > 0
    Xs = (X[live] - fit['mean']) * (1.0 / fit['scale'])
    return FR.evaluate(fit['coef_std'], Xs, (np.asarray(y)[live] != 0).astype(np.float64), r[live], lam)[1]


# ---- features ----

def stage_buffers(n, seed):
    rng = np.random.RandomState(seed)
    prob = rng.uniform(0, 1, n).astype(np.float32)
    score = (rng.randn(n) * 3).astype(np.float32)
    reproj = rng.uniform(0, 1, (n, 5))
    n_mask, n_box = rng.randint(0, 1500, n), rng.randint(0, 1500, n)
    n_both = np.minimum(np.minimum(n_mask, n_box), rng.randint(0, 1500, n))
    counts = np.stack([n_mask, n_box, n_both, rng.randint(0, 8, n)], 1).astype(np.int32)
    view = rng.uniform(0, 1, n).astype(np.float32)
    if n >= 6:                                     # the clamps of prob, an empty mask, an empty union
        prob[:4] = (0.0, 1.0, 5e-7, 1 - 1e-7)
        counts[4, :3] = (0, 12, 0)
        counts[5, :3] = (0, 0, 0)
    return prob, score, reproj, counts, view


def check_features(rt):
    worst = 0.0
    for n, names, extra in ((1, RS.FEATURES, 0), (257, RS.FEATURES, 2), (300, ('score', 'seg_box_iou', 'log_mask'), 1), (64, ('logit_prob',), 0),
                            (65, RS.DEFAULT_FEATURES, 3)):
        prob, score, reproj, counts, view = stage_buffers(n, 7 + n)
        dr = RS.DeviceRescore(rt, n, names)
        dr.ld = dr.F + extra
        dr.X = rt.full((n, dr.ld), -9.0, dtype=torch.float64)
        dr.features(dev(rt, prob), dev(rt, score), dev(rt, reproj), dev(rt, counts), dev(rt, view))
        got = dr.X.cpu().numpy()
        want = FR.features(dr.mask, prob, score, reproj, counts, view)
        assert (got[:, dr.F:] == -9.0).all(), 'a padding column was written'
        for k, name in enumerate(dr.names):
            if name in ('logit_prob', 'log_mask'):
                zero = want[:, k] == 0
                assert (got[zero, k] == 0).all()
                u = ulps(got[~zero, k], want[~zero, k]).max() if (~zero).any() else 0.0
                worst = max(worst, u)
                assert u <= 2, (name, u)
            else:
                assert got[:, k].tobytes() == want[:, k].tobytes(), name
    print('features: log columns within %.1f ulps of the specification' % worst)
    dr = RS.DeviceRescore(rt, 4, ('score', 'view_iou'))
    try:
        dr.features(score=dev(rt, np.zeros(4, np.float32)))
        raise AssertionError('view_iou without the ensemble was accepted')
    except ValueError as e:
        assert '--tta' in str(e)


# ---- apply ----

def check_apply(rt):
    worst = 0.0
    for n in (1, 65, 257, SLICE + 1):
        for F in F_LIST:
            rng = np.random.RandomState(n * 31 + F)
            X, coef = rng.randn(n, F) * 2, rng.randn(F + 1)
            if n > 4:
                X[0], X[1] = 400.0 * np.sign(coef[:F]), -400.0 * np.sign(coef[:F])      # saturates both ways
            nv = n - n // 3
            out, out32 = call_apply(rt, coef, X, n_valid=nv)
            want = FR.apply(coef, X)
            assert (out[nv:] == -3.0).all() and (out32[nv:] == -3.0).all(), 'a row behind n_valid was written'
            rel = np.abs(out[:nv] - want[:nv]) / np.maximum(want[:nv], np.finfo(np.float64).tiny)
            worst = max(worst, rel.max())
            assert rel.max() <= APPLY_REL, (n, F, rel.max())
            assert out32[:nv].tobytes() == out[:nv].astype(np.float32).tobytes()
            assert ((out[:nv] >= 0) & (out[:nv] <= 1)).all()
    out, out32 = call_apply(rt, [1.0, 0.5], np.ones((3, 1)), want32=False)
    assert (out32 == -3.0).all() and (out > 0.8).all()
    print('apply: worst relative difference %.3g (bound %.3g)' % (worst, APPLY_REL))


# ---- fit ----

def check_one_fit(rt, X, y, r, lam, compare, label, max_iter=30):
    """One fit against the specification -> (the device's outputs, |coef_std difference|_inf)."""
    got, want = call_fit(rt, X, y, r, lam, max_iter=max_iter), FR.fit(X, y, r, lam, max_iter=max_iter)
    assert got['status'] == want['status'], (label, RS.status_names(got['status']), RS.status_names(want['status']))
    assert (got['n_rows'], got['n_pos']) == (want['n_rows'], want['n_pos']), label
    k = got['n_iter']
    loss = got['loss'][:k]
    assert np.isnan(got['loss'][k:]).all() and np.isfinite(loss).all(), label
    assert (np.diff(loss) <= 0).all(), (label, 'an accepted loss went up', loss)
    diff = float(np.abs(got['coef_std'] - want['coef_std']).max())
    if got['status'] & ~abi.RESCORE_CONSTANT_COLUMN == 0:
        g = np.abs(gradient(got, X, y, r, lam)).max()
        assert g <= 2 * GTOL, (label, 'gradient', g)
        assert k >= 1 and abs(loss[-1] - want['loss'][want['n_iter'] - 1]) <= 1e-12, label
        live = r > 0
        H = want['hessian']
        A = np.concatenate([(X[live] - want['mean']) / want['scale'], np.ones((int(live.sum()), 1))], 1)
        D = X.shape[1] + 1
        dp_bound = 0.25 * np.sqrt((A * A).sum(1).max()) * (4 * GTOL * np.sqrt(D)) / np.linalg.eigvalsh(H).min()
        dp = np.abs(FR.apply(got['coef'], X[live]) - FR.apply(want['coef'], X[live])).max()
        assert dp <= dp_bound, (label, 'apply outputs of the two models', dp, dp_bound)
        if compare:
            cond = np.linalg.cond(H)
            assert cond < COND_MAX, (label, 'the case is not well-conditioned', cond)
            assert np.allclose(got['mean'], want['mean'], rtol=1e-12, atol=1e-12) and np.allclose(got['scale'], want['scale'], rtol=1e-12), label
            # the raw model is the standardised one, converted
            assert np.allclose(got['coef'][:-1], got['coef_std'][:-1] / got['scale'], rtol=1e-14, atol=0), label
    return got, diff


def check_fit_shapes(rt, n_list=N_LIST):
    """Every shape of the grid against the specification; -> the worst |coef_std difference| of the well-conditioned ones."""
    worst, where = 0.0, None
    for n in n_list:
        for F in F_LIST:
            X, y, r = make_case(n, F, seed=1000 * F + n)
            compare = well_conditioned(n, F)
            got, diff = check_one_fit(rt, X, y, r, LAM, compare, (n, F))
            if compare and got['status'] == 0:
                print('  n %5d F %2d: |coef_std difference| %.3e, %d accepted' % (n, F, diff, got['n_iter']))
                if diff > worst:
                    worst, where = diff, (n, F)
    print('fit: worst |coef_std difference| over the well-conditioned shapes %.3e at n, F = %s (bound %.3e)' % (worst, where, COEF_BOUND))
    assert worst <= COEF_BOUND, ('coef_std', where, worst, COEF_BOUND)
    return worst


def check_equal_bytes(rt):
    for n, F in ((257, 3), (3 * SLICE + 5, 7)):
        X, y, r = make_case(n, F, seed=5)
        a, b = call_fit(rt, X, y, r, LAM), call_fit(rt, X, y, r, LAM)
        assert a['raw'] == b['raw'], (n, F)
        pa, pb = call_apply(rt, a['coef'], X), call_apply(rt, b['coef'], X)
        assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes()


def check_slice_cut(rt):
    """The same weighted rows interleaved with zero-weight rows (which hold NaN: they must not be read into anything) in a larger call:
    other slices, so other orders of the sums -- the coefficients agree within the measured bound, not byte for byte."""
    n, F = SLICE + 300, 7
    X, y, r = make_case(n, F, seed=11, weights='ones')
    rng = np.random.RandomState(12)
    big = 3 * n
    slots = np.sort(rng.permutation(big)[:n])
    Xb, yb, rb = np.full((big, F), np.nan), rng.randint(0, 2, big).astype(np.uint8), np.zeros(big)
    Xb[slots], yb[slots], rb[slots] = X, y, r
    a, b = call_fit(rt, X, y, r, LAM), call_fit(rt, Xb, yb, rb, LAM)
    assert a['status'] == b['status'] == 0 and (a['n_rows'], a['n_pos']) == (b['n_rows'], b['n_pos'])
    diff = np.abs(a['coef_std'] - b['coef_std']).max()
    print('slice cuts: |coef_std difference| %.3e (bound %.3e)' % (diff, COEF_BOUND))
    assert diff <= COEF_BOUND, diff
    return diff


def check_collinear(rt):
    """Two identical columns: the ridge splits the coefficient between them; compared through the gradient and `apply` only."""
    X, y, r = make_case(600, 3, seed=21)
    X = np.concatenate([X, X[:, :1]], 1)
    got, _ = check_one_fit(rt, X, y, r, 1e-3, False, 'collinear')
    assert got['status'] == 0
    assert abs(got['coef_std'][0] - got['coef_std'][3]) <= 1e-6


HALVING_SEEDS = (2, 34, 49)


def halving_case(seed):
    """A few rows of wild scales and weights: the first full Newton steps overshoot and the specification halves."""
    rng = np.random.RandomState(seed)
    n, F = rng.randint(3, 10), rng.randint(1, 4)
    X = rng.randn(n, F) * np.exp(rng.randn(n, 1) * 2)
    y = rng.randint(0, 2, n).astype(np.uint8)
    r = np.exp(rng.randn(n) * 2)
    return X, y, r, 10.0 ** -rng.randint(1, 9)


def check_halving(rt):
    """The halving rule is taken: the fit needs more evaluations than it accepts.  With exactly the evaluations the specification ran it
    converges, with as many as it ACCEPTED it cannot have."""
    for seed in HALVING_SEEDS:
        X, y, r, lam = halving_case(seed)
        want = FR.fit(X, y, r, lam, max_iter=60)
        assert want['status'] == 0 and want['n_eval'] > want['n_iter'], (seed, 'the specification did not halve')
        got, _ = check_one_fit(rt, X, y, r, lam, False, ('halving', seed), max_iter=60)
        assert got['status'] == 0
        short = call_fit(rt, X, y, r, lam, max_iter=want['n_iter'])
        assert short['status'] == abi.RESCORE_NOT_CONVERGED and short['n_iter'] < want['n_iter'], (seed, 'no step was halved')
        assert (np.diff(short['loss'][:short['n_iter']]) <= 0).all()


def check_status_cases(rt):
    X, y, r = make_case(300, 3, seed=31)
    lam = 1e-3
    # every weight 0
    got = call_fit(rt, X, y, np.zeros(300), lam)
    assert got['status'] == abi.RESCORE_NO_ROWS and got['n_rows'] == 0 and got['n_iter'] == 0
    assert (got['coef'] == 0).all() and (got['coef_std'] == 0).all() and (got['mean'] == 0).all() and (got['scale'] == 1).all()
    # one class only: a constant model at the smoothed share
    for yy, rr, XX in ((np.ones(300, np.uint8), r, X), (np.zeros(300, np.uint8), r, X), (np.ones(1, np.uint8), np.array([0.7]), X[:1])):
        got, want = call_fit(rt, XX, yy, rr, lam), FR.fit(XX, yy, rr, lam)
        assert got['status'] & abi.RESCORE_ONE_CLASS and got['status'] == want['status'] and got['n_iter'] == 0
        assert (got['coef'][:-1] == 0).all() and (got['coef_std'][:-1] == 0).all()
        W, Wy = rr[rr > 0].sum(), (rr * yy)[rr > 0].sum()
        q = (Wy + 0.5) / (W + 1.0)
        assert abs(got['coef'][-1] - np.log(q / (1 - q))) <= 1e-12 and got['coef'][-1] == got['coef_std'][-1]
        p = call_apply(rt, got['coef'], XX)[0]
        assert np.allclose(p, q, rtol=1e-12)
    # a constant column: scale 1, coefficient 0, the rest fitted
    Xc = X.copy()
    Xc[:, 1] = 2.5
    got, _ = check_one_fit(rt, Xc, y, r, LAM, False, 'constant column')
    assert got['status'] == abi.RESCORE_CONSTANT_COLUMN and got['scale'][1] == 1 and got['mean'][1] == 2.5 and got['coef_std'][1] == 0
    # a NaN in a weighted row; the same NaN in a zero-weight row
    Xn = X.copy()
    live = np.nonzero(r > 0)[0][5]
    Xn[live, 2] = np.nan
    got = call_fit(rt, Xn, y, r, lam)
    assert got['status'] & abi.RESCORE_NONFINITE and got['n_iter'] == 0 and (got['coef'] == 0).all()
    Xz = X.copy()
    dead = np.nonzero(r == 0)[0][3]
    Xz[dead] = np.nan
    a, b = call_fit(rt, Xz, y, r, LAM), call_fit(rt, X, y, r, LAM)
    assert a['status'] == 0 and a['raw'] == b['raw'], 'a zero-weight row was read into the fit'
    # separable in one dimension, 8 rows: the ridge keeps the coefficients finite
    Xs = np.array([-4., -3, -2, -1, 1, 2, 3, 4])[:, None]
    got, _ = check_one_fit(rt, Xs, (Xs[:, 0] > 0).astype(np.uint8), np.ones(8), 1e-3, False, 'separable')
    assert got['status'] == 0 and np.isfinite(got['coef']).all() and got['coef'][0] > 1
    # one evaluation only
    got = call_fit(rt, X, y, r, lam, max_iter=1)
    assert got['status'] == abi.RESCORE_NOT_CONVERGED and got['n_iter'] == 1 and (got['coef_std'][:-1] == 0).all()
    # n == 0
    got = call_fit(rt, np.zeros((0, 2)), np.zeros(0, np.uint8), np.zeros(0), lam)
    assert got['status'] == abi.RESCORE_NO_ROWS


def check_refusals(lib):
    null = C.c_void_p(0)
    for cls, fn in ((abi.RescoreFeaturesArgs, lib.t3d_rescore_features), (abi.RescoreFitArgs, lib.t3d_rescore_fit),
                    (abi.RescoreApplyArgs, lib.t3d_rescore_apply)):
        a = cls()
        a.struct_size -= 8
        assert fn(C.byref(a), null) == abi.ERR_ABI, cls
    buf = np.zeros(4096)
    D = buf.ctypes.data_as(abi.D)
    y = np.zeros(64, np.uint8).ctypes.data_as(abi.U8)
    i32 = np.zeros(4, np.int32)
    i64 = np.zeros(4, np.int64)

    def fit_args(**kw):
        f = dict(n=8, F=2, ld=2, max_iter=3, reserved=0, X=D, y=y, r=D, lambda_=1e-3, gtol=0.0, workspace=C.c_void_p(buf.ctypes.data),
                 workspace_bytes=buf.nbytes, coef=D, coef_std=D, mean=D, scale=D, loss=D, n_iter=i32.ctypes.data_as(abi.I),
                 status=i32.ctypes.data_as(C.POINTER(C.c_uint32)), n_rows=i64.ctypes.data_as(abi.L), n_pos=i64.ctypes.data_as(abi.L))
        f.update(kw)
        return abi.RescoreFitArgs(**f)
    refuse = lambda want, **kw: (lib.t3d_rescore_fit(C.byref(fit_args(**kw)), null), want, kw)
    for got, want, kw in (refuse(-2, F=16), refuse(-2, F=0), refuse(-2, n=-1), refuse(-2, ld=1), refuse(-1, lambda_=0.0), refuse(-1, lambda_=-1.0),
                          refuse(-1, lambda_=float('nan')), refuse(-1, gtol=-1.0), refuse(-1, max_iter=-1), refuse(-1, reserved=1),
                          refuse(-1, X=abi.D()), refuse(-1, r=abi.D()), refuse(-1, y=abi.U8()), refuse(-1, coef=abi.D()), refuse(-1, loss=abi.D()),
                          refuse(-1, workspace=C.c_void_p(0)), refuse(-1, workspace_bytes=64), refuse(-1, workspace=C.c_void_p(buf.ctypes.data + 4))):
        assert got == want, (got, want, kw)
    fz = np.zeros(64, np.float32).ctypes.data_as(abi.F)

    def feat(**kw):
        f = dict(n=4, ld=7, feature_mask=127, prob=fz, score=fz, reproj=D, counts=i32.ctypes.data_as(abi.I), view_iou=fz, X=D)
        f.update(kw)
        return lib.t3d_rescore_features(C.byref(abi.RescoreFeaturesArgs(**f)), null)
    assert feat(feature_mask=0) == -1 and feat(feature_mask=128) == -1 and feat(X=abi.D()) == -1 and feat(view_iou=abi.F()) == -1
    assert feat(prob=abi.F()) == -1 and feat(counts=abi.I()) == -1 and feat(ld=6) == -2 and feat(n=-1) == -2
    assert feat(n=0) == 0 and feat(n=0, feature_mask=63, view_iou=abi.F()) == 0

    def app(**kw):
        f = dict(n=4, n_valid=4, F=2, ld=2, reserved=0, X=D, coef=D, out=D, out32=fz)
        f.update(kw)
        return lib.t3d_rescore_apply(C.byref(abi.RescoreApplyArgs(**f)), null)
    assert app(X=abi.D()) == -1 and app(coef=abi.D()) == -1 and app(out=abi.D()) == -1 and app(reserved=2) == -1
    assert app(F=16) == -2 and app(F=0) == -2 and app(ld=1) == -2 and app(n_valid=5) == -2 and app(n=-1, n_valid=0) == -2
    assert app(n_valid=0) == 0


# ---- statistics ----

RECOVERY_SEEDS = (101, 202, 303)


def recovery_case(seed, n=20000, F=4):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, F) * np.array([1.0, 2.0, 0.5, 1.5])[:F] + np.array([0.5, -1.0, 2.0, 0.0])[:F]
    truth = np.array([0.8, -0.4, 1.2, 0.3, -0.5])
    y = (rng.uniform(size=n) < FR.apply(truth, X)).astype(np.uint8)
    return X, y, np.ones(n), truth


def check_recovery(fit_fn):
    """20 000 rows drawn from a known model, a ridge too small to matter: every coefficient within 5 standard errors of the truth.
    fit_fn(X, y, r, lam) -> dict with 'coef' and 'status'."""
    for seed in RECOVERY_SEEDS:
        X, y, r, truth = recovery_case(seed)
        got = fit_fn(X, y, r, 1e-8)
        assert got['status'] == 0, RS.status_names(got['status'])
        se = FR.standard_errors(X, r, got['coef'])
        dev_ = np.abs(got['coef'] - truth) / se
        print('recovery seed %d: |coef - truth| / se = %s' % (seed, np.round(dev_, 2)))
        assert (dev_ <= 5).all(), (seed, dev_)


# ---- the model file ----

def check_model_round_trip(rt, tmp_path):
    X, y, r = make_case(500, 3, seed=41)
    names = ('score', 'reproj_iou', 'log_mask')
    dr = RS.DeviceRescore(rt, 500, names)
    dr.X.copy_(dev(rt, X))
    dr.fit(dev(rt, y), dev(rt, r), 1e-3)
    f = dr.fetch_fit()
    assert f['status'] == 0
    dr.apply()
    first = dr.out.cpu().numpy().copy(), dr.out32.cpu().numpy().copy()
    m = RS.Model(names, f['coef'], f['coef_std'], f['mean'], f['scale'], target='overlap', threshold=0.25, lam=1e-3, classes=['chair', 'bed'],
                 n_rows=f['n_rows'], n_pos=f['n_pos'], loss=f['loss'][f['n_iter'] - 1], status=RS.status_names(f['status']), n_iter=f['n_iter'],
                 holdout={'mean_ap_prob': 0.5})
    path = str(tmp_path / 'model.json')
    m.save(path)
    back = RS.Model.load(path)
    assert back.to_dict() == m.to_dict() and np.asarray(back.coef).tobytes() == f['coef'].tobytes()
    other = RS.DeviceRescore(rt, 500, names)
    other.X.copy_(dev(rt, X))
    other.load(back)
    other.apply()
    assert other.out.cpu().numpy().tobytes() == first[0].tobytes() and other.out32.cpu().numpy().tobytes() == first[1].tobytes()
    try:
        RS.DeviceRescore(rt, 4, ('score',)).load(back)
        raise AssertionError('a model of other features was loaded')
    except ValueError:
        pass


# ---- flows: detect and autolabel with a model -------------------------------------------------------------------------------------

def hand_model(names=('score', 'reproj_iou'), coef=(0.05, 6.0, -2.0)):
    """A model written down by hand (the golden scenes run on the graph's initial weights: nothing a fit could learn from)."""
    return RS.Model(names, coef)


def rescore_of(model, prob, d, rows):
    """The specification's rescore_prob of rows of a Decoded, from what the records say."""
    reproj = np.zeros((len(rows), 5))
    reproj[:, 4] = d.reproj_iou[rows]
    counts = np.stack([d.n_mask[rows], d.n_box[rows], d.n_both[rows], d.flags[rows]], 1)
    view = None if d.view_iou is None else d.view_iou[rows]
    X = FR.features(model.mask, np.asarray(prob, np.float32), d.score[rows].astype(np.float32), reproj, counts, view)
    return FR.apply(model.coef, X)


def check_flag_errors(rt, root, model_path):
    import detect_check as DC
    from transferable3d_amd import autolabel as AL, detect as DT
    ids, folder, idx, dets = DC.write_data_set(root)
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS
    sweep = ['--sweep', '--sweep_nms_iou', 'off', '0.25']
    for bad in (['--min_rescore', '0.5'], ['--rescore', model_path, '--rescore_fit', str(root / 'm.json')], ['--rescore', model_path] + sweep,
                ['--rescore_fit', str(root / 'm.json')] + sweep, ['--rescore_lambda', '0.1'], ['--rescore_features', 'score'],
                ['--rescore_target', 'tp'], ['--rescore_holdout', '0.2'], ['--rescore_classes', 'chair'], ['--rescore', model_path, '--min_rescore', '1.5'],
                ['--rescore', model_path, '--min_rescore', '-0.1'], ['--rescore_fit', str(root / 'm.json'), '--rescore_holdout', '1.0'],
                ['--rescore_fit', str(root / 'm.json'), '--rescore_lambda', '0'], ['--rescore_fit', str(root / 'm.json'), '--nms_iou', '0.25'],
                ['--rescore_fit', str(root / 'm.json'), '--rescore_features', 'view_iou']):
        try:
            DT.main(base + bad, rt=rt, log=lambda *a: None)
        except SystemExit as e:
            assert e.code == 2, bad
        else:
            raise AssertionError('accepted: %s' % ' '.join(bad))
    views = str(root / 'views.json')
    RS.Model(('score', 'view_iou'), [1.0, 1.0, 0.0]).save(views)
    try:
        DT.Detector(DC.TS.build_flags(DC.MODEL_FLAGS), rt=rt, rescore=views)
        raise AssertionError('view_iou without tta was accepted')
    except ValueError as e:
        assert '--tta' in str(e)
    try:
        AL.main(['--dataset_dir', str(root), '--idx_path', idx, '--classes', 'chair', '--out_dir', str(root / 'o'), '--min_rescore', '0.5'] + DC.MODEL_FLAGS,
                rt=rt, log=lambda *a: None)
        raise AssertionError('autolabel took --min_rescore without --rescore')
    except SystemExit as e:
        assert e.code == 2
    return ids, folder, idx, dets, base


def check_detect_flow(rt, root):
    """detect with --rescore on the golden scenes: rescore_prob in records, legends, JSON rows and the last column of the result files;
    without the flags no output names it."""
    import json
    import detect_check as DC
    import consistency_check as CK
    from transferable3d_amd import detect as DT
    model = hand_model()
    model_path = str(root / 'hand.json')
    model.save(model_path)
    ids, folder, idx, dets, base = check_flag_errors(rt, root, model_path)
    scenes = CK.scenes_with_sizes(root, ids)
    flags = lambda: DC.TS.build_flags(DC.MODEL_FLAGS)
    plain = DT.Detector(flags(), rt=rt, consistency=True).detect(scenes, dets, scene_ids=ids)
    det = DT.Detector(flags(), rt=rt, rescore=model_path)
    got = det.detect(scenes, dets, scene_ids=ids)
    flat, flat0 = [r for recs in got for r in recs], [r for recs in plain for r in recs]
    assert len(flat) == len(flat0) > 4
    for r, r0 in zip(flat, flat0):
        assert 'rescore_prob' not in r0 and set(r) == set(r0) | {'rescore_prob'}
        for k in r0:
            assert np.array_equal(r[k], r0[k]), k                 # prob stays the 2-D detector's; everything else is untouched
        X = np.array([[np.float64(np.float32(r['score'])), r['reproj_iou']]])
        want = FR.apply(model.coef, X)[0]
        assert abs(r['rescore_prob'] - want) <= APPLY_REL * want, (r['rescore_prob'], want)
    assert len(set(round(r['rescore_prob'], 6) for r in flat)) > 2
    # the command line: the last column of the result files, the JSON rows, the legends
    res, cj, vis = str(root / 'res'), str(root / 'rows.json'), str(root / 'vis')
    lines = []
    p = DT.main(base + ['--rescore', model_path, '--result_dir', res, '--consistency_json', cj, '--vis_dir', vis, '--official_eval'], rt=rt, log=lines.append)
    assert [float(v) for v in p[9]] == [r['rescore_prob'] for r in flat]
    files = DC.read_results(res)
    want_files = DC.record_lines(ids, [[dict(r, prob=r['rescore_prob']) for r in recs] for recs in got])
    assert {c: t for c, t in files.items() if t} == want_files
    rows = json.load(open(cj))
    assert [row['rescore_prob'] for row in rows] == [r['rescore_prob'] for r in flat] and [row['prob'] for row in rows] == [r['prob'] for r in flat]
    legends = [json.load(open(os.path.join(vis, f))) for f in sorted(os.listdir(vis)) if f.endswith('.json')]
    shown = [b for l in legends for b in l['boxes'] if b['kind'] != 'gt']
    assert shown and all('rescore_prob' in b for b in shown)
    assert any(l.startswith('Mean AP Score') for l in lines)
    # without the flags nothing names it
    q = DT.main(base + ['--result_dir', str(root / 'res0'), '--consistency', '--consistency_json', str(root / 'rows0.json')], rt=rt, log=lambda *a: None)
    assert [float(v) for v in q[9]] == [r['prob'] for r in flat0] and q.decoded.rescore_prob is None
    assert {c: t for c, t in DC.read_results(str(root / 'res0')).items() if t} == DC.record_lines(ids, plain)
    assert all('rescore_prob' not in row for row in json.load(open(root / 'rows0.json')))
    return flat


def check_accept_and_ranking(rt, root):
    """One object reported twice, the worse 3-D box (by reproj_iou) with the better 2-D confidence.  By `prob` it suppresses the other;
    with a model that reads reproj_iou the suppression, the box voting and Soft-NMS rank by rescore_prob, and min_rescore between the two
    values rejects the worse one in front of the NMS groups."""
    import detect_check as DC
    import consistency_check as CK
    from transferable3d_amd import detect as DT
    ids, folder, idx, dets = DC.write_data_set(root)
    scenes = CK.scenes_with_sizes(root, ids)[:1]
    name, box, _ = next(d for d in dets[0] if d != DC.SPARSE)
    pair = [tuple(box), tuple(np.asarray(box) + (6.0, 4.0, 6.0, 4.0))]
    model = RS.Model(('reproj_iou',), [8.0, -2.0])
    run = lambda probs, **kw: DT.Detector(DC.TS.build_flags(DC.MODEL_FLAGS), rt=rt, **kw).detect(
        scenes, [[(name, pair[0], probs[0]), (name, pair[1], probs[1])]], scene_ids=ids[:1])[0]
    both = run((0.9, 0.8), rescore=model)
    assert len(both) == 2
    v = [r['reproj_iou'] for r in both]
    assert v[0] != v[1]
    worse = int(v[1] < v[0])
    probs = (0.9, 0.8) if worse == 0 else (0.8, 0.9)
    both = run(probs, rescore=model)
    rp = [r['rescore_prob'] for r in both]
    assert rp[1 - worse] > rp[worse] and both[worse]['prob'] == 0.9
    by_prob = run(probs, nms_iou=0.05)
    assert len(by_prob) == 1 and np.array_equal(by_prob[0]['box2d'], pair[worse])
    by_model = run(probs, nms_iou=0.05, rescore=model)
    assert len(by_model) == 1 and np.array_equal(by_model[0]['box2d'], pair[1 - worse]) and by_model[0]['rescore_prob'] == rp[1 - worse]
    by_score = run(probs, nms_iou=0.05, nms_score='score', rescore=model), run(probs, nms_iou=0.05, nms_score='score')
    assert np.array_equal(by_score[0][0]['box2d'], by_score[1][0]['box2d'])                       # --nms_score score is unchanged
    fused = run(probs, nms_iou=0.05, nms_fuse=True, rescore=model)
    assert len(fused) == 1 and np.array_equal(fused[0]['box2d'], pair[1 - worse]) and fused[0]['votes'] == 1
    soft = run(probs, soft_nms='gaussian', rescore=model)
    assert len(soft) == 2
    assert soft[1 - worse]['soft_prob'] == float(np.float32(rp[1 - worse])) and soft[1 - worse]['decays'] == 0
    assert soft[worse]['soft_prob'] < float(np.float32(rp[worse])) and soft[worse]['decays'] == 1
    cut = (rp[0] + rp[1]) / 2.0
    lines = []
    kept = run(probs, nms_iou=0.05, rescore=model, min_rescore=cut, log=lines.append)
    assert len(kept) == 1 and np.array_equal(kept[0]['box2d'], pair[1 - worse])
    assert lines[0] == 'consistency: kept 1 of 2 (rescore_prob < %g: 1)' % cut and 'kept 1 of 1' in lines[1], lines
    try:
        run(probs, min_rescore=0.5)
        raise AssertionError('min_rescore without a model was accepted')
    except ValueError:
        pass
    return rp


def check_autolabel_flow(rt, root):
    import detect_check as DC
    from transferable3d_amd import autolabel as AL
    ids, folder, idx, dets = DC.write_data_set(root)
    model_path = str(root / 'auto_model.json')
    RS.Model(('reproj_iou', 'mask_in_box'), [6.0, 1.0, -2.5]).save(model_path)
    classes = sorted(set(d[0] for scene in dets for d in scene))
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--classes'] + classes
    first = AL.main(base + ['--out_dir', str(root / 'a0'), '--rescore', model_path] + DC.MODEL_FLAGS, rt=rt, log=lambda *a: None)
    values = sorted(r['rescore_prob'] for r in first['_records'] if r['detected'])
    assert first['rescore'] == {'features': ['reproj_iou', 'mask_in_box'], 'min_rescore': None} and len(values) > 4
    cut = (values[len(values) // 2 - 1] + values[len(values) // 2]) / 2.0
    lines = []
    s = AL.main(base + ['--out_dir', str(root / 'a1'), '--rescore', model_path, '--min_rescore', repr(cut), '--score_against_labels'] + DC.MODEL_FLAGS,
                rt=rt, log=lines.append)
    det = [r for r in s['_records'] if r['detected']]
    assert all(r['accepted'] == (r['rescore_prob'] >= cut) for r in det)
    n_rej = sum(c['rejected_by']['min_rescore'] for c in s['classes'].values())
    assert n_rej == sum(1 for r in det if not r['accepted']) >= 2 and sum(c['accepted'] for c in s['classes'].values()) >= 2
    assert any('by --min_rescore' in l for l in lines), lines
    by = [v['min_rescore'] for v in s['score_against_labels'].values()]
    assert sum(b['accepted']['n'] for b in by) == sum(1 for r in det if r['accepted'])
    plain = AL.main(base + ['--out_dir', str(root / 'a2')] + DC.MODEL_FLAGS, rt=rt, log=lambda *a: None)
    assert 'rescore' not in plain and all('rescore_prob' not in r for r in plain['_records'])


def check_fit_command(rt, root):
    """detect --rescore_fit end to end on the duplicated golden scenes (the graph's initial weights: what is learnt means nothing, the
    flow is what is checked): the log lines, the model file, the held-out report, and the model applied by a second run."""
    import json
    import detect_check as DC
    import nms_check as NC
    from transferable3d_amd import detect as DT
    ids, folder, idx, dets = NC.write_duplicated(root)
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS
    path = str(root / 'fitted.json')
    lines = []
    model = DT.main(base + ['--rescore_fit', path, '--rescore_features', 'score', 'reproj_iou', 'log_mask', '--rescore_holdout', '0.5'], rt=rt, log=lines.append)
    assert isinstance(model, RS.Model) and model.features == ['score', 'reproj_iou', 'log_mask']
    fit_line = [l for l in lines if l.startswith('rescore: fit on ')]
    assert len(fit_line) == 1 and ' classes, ' in fit_line[0], lines
    assert any(l.startswith('rescore: coefficients per standardised feature: score ') for l in lines)
    back = RS.Model.load(path)
    assert back.to_dict() == json.loads(json.dumps(model.to_dict()))
    assert back.holdout is not None and set(back.holdout['classes']) == set(back.classes) and len(back.holdout['reliability']) == 10
    assert any(l.startswith('rescore: held-out mean AP: by prob ') for l in lines)
    for c, v in back.holdout['classes'].items():
        assert 0.0 <= v['ap_prob'] <= 1.0 and 0.0 <= v['ap_rescore_prob'] <= 1.0
    whole = DT.main(base + ['--rescore_fit', str(root / 'whole.json'), '--rescore_holdout', '0', '--rescore_target', 'tp'], rt=rt, log=lines.append)
    assert whole.holdout is None and whole.target == 'tp' and whole.features == list(RS.DEFAULT_FEATURES) and whole.n_rows >= model.n_rows
    p = DT.main(base + ['--rescore', path], rt=rt, log=lambda *a: None)
    assert p.decoded.rescore_prob is not None and np.isfinite(p.decoded.rescore_prob).all()
    return lines


def check_constructed_case(rt):
    """Parallel to the row of chairs: every detection has prob 0.9; the ones on an object have a high reproj_iou, the background ones a
    low one.  On the held-out half the AP by prob is whatever the tie order gives, and the AP by rescore_prob is 1.0 -- a property of
    the construction (the feature separates the two kinds), not of any data."""
    from transferable3d_amd import evaluate_sunrgbd as ES
    rng = np.random.RandomState(5)
    n_img = 60
    img, on, tx = [], [], []
    for i in range(n_img):
        for k in range(2):                                       # two objects per image, 4 m apart; per object a background box first
            img += [i, i]
            on += [0, 1]
            tx += [4.0 * k + 2.0, 4.0 * k]
    img, on, tx = np.array(img), np.array(on, bool), np.array(tx)
    n = len(img)
    one = np.ones(n)
    boxes = lambda sel, conf: ES.boxes_from_label_format(img[sel], one[sel], one[sel], one[sel], tx[sel], 0.5 * one[sel], 3 * one[sel], 0 * one[sel], conf)
    gt = dict(boxes(on, one[on]), classname=['chair'] * int(on.sum()))
    reproj = np.zeros((n, 5))
    reproj[:, 4] = np.where(on, rng.uniform(0.7, 0.9, n), rng.uniform(0.05, 0.3, n))
    prob = np.full(n, 0.9, np.float32)
    fit_half = img < n_img // 2
    dr = RS.DeviceRescore(rt, n, ('logit_prob', 'reproj_iou'))
    dr.features(prob=dev(rt, prob), reproj=dev(rt, reproj))
    dr.fit(dev(rt, on.astype(np.uint8)), dev(rt, fit_half.astype(np.float64)), 1e-3)
    dr.apply()
    f = dr.fetch_fit()
    assert f['status'] == abi.RESCORE_CONSTANT_COLUMN and f['coef_std'][0] == 0 and f['coef_std'][1] > 0, (RS.status_names(f['status']), f['coef_std'])
    rescored = dr.out.cpu().numpy()
    held = ~fit_half
    gt_held = ES.select_boxes(gt, np.asarray(gt['image']) >= n_img // 2)
    ap = {k: ES.compute_pr_curve_3d('chair', boxes(held, conf[held]), gt_held, None, 0.25, rt)['apScore']
          for k, conf in (('prob', prob.astype(np.float64)), ('rescore_prob', rescored))}
    print('constructed case: held-out AP by prob %.4f, by rescore_prob %.4f' % (ap['prob'], ap['rescore_prob']))
    assert ap['rescore_prob'] == 1.0 and ap['prob'] < 1.0, ap
