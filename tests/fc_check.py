"""Shared cases of the FC kernel tests (tests/test_kernels_fc_gpu.py on libt3d.so, tests/test_kernels_fc_cpu.py on fake_t3d.FakeLib).

csrc/fc_dev.h holds the three fully-connected bodies (fc_fwd_body, fc_bwd_body, fc_dinput_body); they run stand-alone (csrc/fc.hip, 512
threads, RBT = 1 for B <= 32, RBT = MAXRB above), paired (csrc/pair.hip k_small_pair) and as riders (csrc/rider_dev.h, 256 threads), and
the three forms promise the same bits.  The cases here sit on the bodies' edge logic: clamped addresses and masked values, the 16-byte
k-loop handing over to the scalar one at `gfull`, k-groups dealt to waves in runs, a k-group that straddles in | in2, partly filled row
blocks, a ragged last column block, the prefetched and the looped dW.  Every case is in tests/rider_check.py's format -- a function
`case(bufs) -> [(entry point, argument struct)]`, every written tensor from `bufs.out` (sentinel-filled, fenced by guard bands) -- so the
same case runs stand-alone against the fp64 specification (rider_check.ORACLE_TOL, no other bound), as a one-op rider set, and in a pair.

Inputs with a row stride carry 1e3 in their padding columns, so a read through a wrong stride or past K is not a small error.  Saved
activations of a backward case (y, mean, invstd) are inputs, identical on both sides; where the backward depends on an activation branch
the fp64 z keeps 64 fp32 spacings from 0 (`nudge_margin`, `margin_violations`)."""
import ctypes as C

import numpy as np

import rider_check as rc
from fake_t3d import FakeLib, arr
from rider_check import (Bufs, Env, ERR_ARG, ERR_SHAPE, REPS, assert_same_bits, check_against_oracle, check_guards,      # noqa: F401
                         check_set_alone, run_alone, run_apart, small_op)
from transferable3d_amd import abi
from transferable3d_amd.abi import fptr

SPEC = Env(FakeLib(), 'cpu')
EPS, ALPHA, KEEP, DECAY = 1e-3, 0.2, 0.7, 0.6
MARGIN_ULPS = 64
STATS = {}      # (kind, output) -> [largest error, bound there, largest error / bound, case]: filled by check_case / check_pair on the device


def _rows(r, B, n, ld, scale=1.0):
    """[B, ld]: n random columns, 1e3 in the padding columns"""
    x = np.full((B, max(ld, 1)), 1e3, np.float32)
    x[:, :n] = r.normal(size=(B, n)) * scale
    return x


def _rs(seed, *dims):
    return np.random.RandomState(seed + sum(int(d) * m for d, m in zip(dims, (1009, 31, 7, 3, 1))))


class _Tag:
    """A Bufs whose output names carry a prefix: the two ops of a pair built from two one-op cases."""

    def __init__(self, b, tag):
        self.b, self.tag, self.dev = b, tag, b.dev

    def inp(self, a):
        return self.b.inp(a)

    def out(self, name, *a, **k):
        return self.b.out(self.tag + name, *a, **k)


# ---- the three kinds -----------------------------------------------------------------------------------------------------------------------
def fwd_case(B, K, N, ld_in=None, K2=0, ld_out=None, bn='train', act='relu', drop=False, bias=True, add=None, identity=False, unbiased=1,
             save_y=True, seed=21):
    """t3d_fc_fwd.  bn: 'train' | 'eval' | None; add = (add_n, ld_add); identity: w == NULL (K == N)."""
    ld_in, ld_out, Kt = (K if ld_in is None else ld_in), (N if ld_out is None else ld_out), K + K2
    r = _rs(seed, B, K, N, K2, ld_in)
    x, x2 = _rows(r, B, K, ld_in), (_rows(r, B, K2, K2 + 3) if K2 else None)
    w, bv = (r.normal(size=(Kt, N)) / np.sqrt(Kt)).astype(np.float32), (r.normal(size=N) * 0.1).astype(np.float32)
    gamma, beta = (0.5 + r.uniform(size=N)).astype(np.float32), (r.normal(size=N) * 0.1).astype(np.float32)
    mm, mv = (r.normal(size=N) * 0.1).astype(np.float32), (0.5 + r.uniform(size=N)).astype(np.float32)
    mask = (r.uniform(size=(B, N)) < KEEP).astype(np.float32)
    addv = _rows(r, B, add[0], add[1]) if add else None

    def case(b):
        a = abi.FcFwdArgs()
        a.in_, a.ld_in, a.K = fptr(b.inp(x)), ld_in, K
        if K2:
            a.in2, a.ld_in2, a.K2 = fptr(b.inp(x2)), K2 + 3, K2
        if not identity:
            a.w = fptr(b.inp(w))
        if bias:
            a.bias = fptr(b.inp(bv))
        if bn:
            a.gamma, a.beta = fptr(b.inp(gamma)), fptr(b.inp(beta))
            a.moving_mean, a.moving_var = fptr(b.out('mm', N, init=mm)), fptr(b.out('mv', N, init=mv))
            a.mean, a.invstd = fptr(b.out('mean', N)), fptr(b.out('invstd', N))
        a.decay, a.eps, a.is_training, a.unbiased_ema = fptr(b.inp(np.array([DECAY], np.float32))), EPS, int(bn != 'eval'), unbiased
        a.act, a.leaky_alpha = abi.ACT_BY_NAME[act], ALPHA
        if drop:
            a.drop_mask, a.keep_prob = fptr(b.inp(mask)), KEEP
        if add:
            a.add_in, a.ld_add, a.add_n = fptr(b.inp(addv)), add[1], add[0]
        if bn or save_y:
            a.y = fptr(b.out('y', (B, N)))
        a.out, a.ld_out, a.B, a.N = fptr(b.out('out', (B, ld_out))), ld_out, B, N
        return [('t3d_fc_fwd', a)]
    case.B, case.kind = B, 'fwd'
    return case


def _z_and_scale(y, mean, invstd, gamma, beta, bn):
    y = y.astype(np.float64)
    if not bn:
        return y, np.abs(y)
    xg = (y - mean.astype(np.float64)) * invstd.astype(np.float64) * gamma.astype(np.float64)
    return xg + beta.astype(np.float64), np.abs(xg) + np.abs(beta.astype(np.float64))


def margin_violations(y, mean, invstd, gamma, beta, bn):
    """elements whose fp64 z lies within MARGIN_ULPS fp32 spacings (of |xhat gamma| + |beta|, or of |y| without BN) of 0"""
    z, scale = _z_and_scale(y, mean, invstd, gamma, beta, bn)
    return np.abs(z) < MARGIN_ULPS * np.spacing(np.maximum(scale, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def nudge_margin(y, mean, invstd, gamma, beta, bn):
    """y with every violating element moved (mean / invstd are saved inputs and stay): regenerated, never skipped"""
    y = y.copy()
    for _ in range(20):
        bad = margin_violations(y, mean, invstd, gamma, beta, bn)
        if not bad.any():
            return y
        y[bad] += np.float32(1e-2) * (1 + np.abs(y[bad]))
    raise AssertionError('the margin could not be restored')


def bwd_case(B, K, N, ld_in=None, K2=0, src='dout', N_next=96, ld_dout=None, bn='train', act='relu', drop=False, dw=True, dparams=True, seed=22):
    """t3d_fc_bwd.  src: 'dout' (given, rows ld_dout apart) | 'next' (dy_next . w_next^T); bn: 'train' | 'frozen' | None."""
    ld_in, ld_dout, Kt = (K if ld_in is None else ld_in), (N if ld_dout is None else ld_dout), K + K2
    r = _rs(seed, B, K, N, K2, ld_in + N_next * (src == 'next'))
    y = r.normal(size=(B, N)).astype(np.float32)
    gamma, beta = (0.5 + r.uniform(size=N)).astype(np.float32), (r.normal(size=N) * 0.1).astype(np.float32)
    mean, invstd = y.mean(0).astype(np.float32), (1.0 / np.sqrt(y.var(0) + EPS)).astype(np.float32)
    if act in ('relu', 'leaky_relu'):
        y = nudge_margin(y, mean, invstd, gamma, beta, bool(bn))
    mask = (r.uniform(size=(B, N)) < KEEP).astype(np.float32)
    x, x2 = _rows(r, B, K, ld_in), (_rows(r, B, K2, K2 + 3) if K2 else None)
    dout = _rows(r, B, N, ld_dout)
    dyn, wn = r.normal(size=(B, N_next)).astype(np.float32), (r.normal(size=(N, N_next)) / np.sqrt(N_next)).astype(np.float32)
    keep = (r.normal(size=N)).astype(np.float32)      # what dgamma / dbeta hold before a frozen call, which leaves them alone

    def case(b):
        a = abi.FcBwdArgs()
        if src == 'next':
            a.dy_next, a.w_next, a.N_next = fptr(b.inp(dyn)), fptr(b.inp(wn)), N_next
        else:
            a.dout, a.ld_dout = fptr(b.inp(dout)), ld_dout
        a.in_, a.ld_in, a.K = fptr(b.inp(x)), ld_in, K
        if K2:
            a.in2, a.ld_in2, a.K2 = fptr(b.inp(x2)), K2 + 3, K2
        a.y, a.ld_out = fptr(b.inp(y)), N
        if bn:
            a.gamma, a.beta, a.mean, a.invstd = fptr(b.inp(gamma)), fptr(b.inp(beta)), fptr(b.inp(mean)), fptr(b.inp(invstd))
        a.bn_training, a.act, a.leaky_alpha = int(bn != 'frozen'), abi.ACT_BY_NAME[act], ALPHA
        if drop:
            a.drop_mask, a.keep_prob = fptr(b.inp(mask)), KEEP
        a.dy = fptr(b.out('dy', (B, N)))
        if dw:
            a.dw = fptr(b.out('dw', (Kt, N)))
        if dparams:
            a.dbias = fptr(b.out('db', N))
            if bn:
                init = keep if bn == 'frozen' else None
                a.dgamma, a.dbeta = fptr(b.out('dgamma', N, init=init)), fptr(b.out('dbeta', N, init=init))
        a.B, a.N = B, N
        return [('t3d_fc_bwd', a)]
    case.B, case.kind = B, 'bwd'
    case.facts = dict(y=y, mean=mean, invstd=invstd, gamma=gamma, beta=beta, bn=bool(bn), act=act)
    return case


def dinput_case(B, N, K, alpha=1.0, ld_add=None, ld_din=None, fused=None, dparams=True, seed=23):
    """t3d_fc_dinput: din = alpha dy . w^T (+ add_in).  fused: None | 'train' | 'frozen' -- the pooled batch-norm backward on din's
    columns (bn_ld_pooled = K + 5; frozen: bn_gamma = bn_mean = bn_invstd = NULL, as the launcher allows)."""
    ld_din = K if ld_din is None else ld_din
    r = _rs(seed, B, K, N, ld_din, int(alpha * 4))
    dy, w = r.normal(size=(B, N)).astype(np.float32), (r.normal(size=(K, N)) / np.sqrt(N)).astype(np.float32)
    addv = _rows(r, B, K, ld_add) if ld_add else None
    pooled = _rows(r, B, K, K + 5)
    pooled[:, :K] = np.maximum(pooled[:, :K], 0)
    ysel = r.normal(size=(B, K)).astype(np.float32)
    g4 = [(0.5 + r.uniform(size=K)).astype(np.float32), r.normal(size=K).astype(np.float32), (0.5 + r.uniform(size=K)).astype(np.float32),
          r.normal(size=K).astype(np.float32)]      # gamma, mean, invstd, scale

    def case(b):
        a = abi.FcDinputArgs()
        a.dy, a.N, a.w, a.alpha = fptr(b.inp(dy)), N, fptr(b.inp(w)), alpha
        if ld_add:
            a.add_in, a.ld_add = fptr(b.inp(addv)), ld_add
        a.din, a.ld_din, a.B, a.K = fptr(b.out('din', (B, ld_din))), ld_din, B, K
        if fused:
            a.bn_pooled, a.bn_ld_pooled, a.bn_ysel = fptr(b.inp(pooled)), K + 5, fptr(b.inp(ysel))
            a.bn_dpool, a.bn_count, a.bn_scale = fptr(b.out('dpool', (B, K))), B * 1024, fptr(b.inp(g4[3]))
            a.bn_frozen = int(fused == 'frozen')
            if fused == 'train':
                a.bn_gamma, a.bn_mean, a.bn_invstd = fptr(b.inp(g4[0])), fptr(b.inp(g4[1])), fptr(b.inp(g4[2]))
                if dparams:
                    a.bn_dgamma, a.bn_dbeta = fptr(b.out('bn_dg', K)), fptr(b.out('bn_db', K))
            a.bn_coef = fptr(b.out('bn_coef', (3, K)))
        return [('t3d_fc_dinput', a)]
    case.B, case.kind = B, 'dinput'
    return case


def bn_bwd_frozen_case(N, dense, B=8, n_tiles=8, seed=24):
    """t3d_bn_bwd_finalize, frozen, with gamma = mean = invstd = NULL (t3d.h: `scale` is what a frozen call uses): coef = (scale, 0, 0);
    the pooled form also writes dpool."""
    r = _rs(seed, N, n_tiles, int(dense))
    s1, s2 = r.normal(size=(n_tiles, N)).astype(np.float32), r.normal(size=(n_tiles, N)).astype(np.float32)
    scale, dpin, ysel = r.normal(size=N).astype(np.float32), _rows(r, B, N, N + 3), r.normal(size=(B, N)).astype(np.float32)
    pooled = _rows(r, B, N, N + 5)
    pooled[:, :N] = np.maximum(pooled[:, :N], 0)

    def case(b):
        a = abi.BnBwdFinalizeArgs()
        if dense:
            a.psum_dz, a.psum_dzy, a.n_tiles = fptr(b.inp(s1)), fptr(b.inp(s2)), n_tiles
        else:
            a.dpool_in, a.ld_dpool_in, a.pooled, a.ld_pooled = fptr(b.inp(dpin)), N + 3, fptr(b.inp(pooled)), N + 5
            a.ysel, a.dpool, a.B = fptr(b.inp(ysel)), fptr(b.out('dpool', (B, N))), B
        a.count, a.N, a.scale, a.frozen, a.coef = n_tiles * 128, N, fptr(b.inp(scale)), 1, fptr(b.out('coef', (3, N)))
        return [('t3d_bn_bwd_finalize', a)]
    case.kind = 'bn_bwd'
    return case


# ---- part 1: the case tables ------------------------------------------------------------------------------------------------------------------
CASES = {}      # id -> (factory, kwargs)


def _add(cid, factory, **kw):
    assert cid not in CASES, cid
    CASES[cid] = (factory, kw)


ROW_B = [1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128]
COLS = [1, 31, 32, 33, 67]
RED = [(3, 3, 0), (8, 8, 0), (13, 13, 0), (60, 60, 0), (60, 60, 10), (64, 68, 10), (68, 70, 0), (72, 72, 0), (1096, 1096, 0)]      # (K, ld_in, K2)
WT_RED = [3, 9, 67, 96, 100]      # reduction length = ldw of wave_gemm<true>: scalar, scalar, scalar, vector only, vector then a half group
FORM_B = [31, 97]
FUSED_B, FUSED_K = [1, 31, 33, 128], [33, 96]

for _B in ROW_B:      # row edges: bn train + relu + dropout, K = 64, N = 33, ld_out = 40
    _add('fwd-rows-B%d' % _B, fwd_case, B=_B, K=64, N=33, ld_out=40, drop=True)
    _add('bwd-rows-B%d' % _B, bwd_case, B=_B, K=64, N=33, drop=True)
    _add('dinput-rows-B%d' % _B, dinput_case, B=_B, N=64, K=33, ld_din=40)
for _N in COLS:       # column edges at B = 33 (for dinput the column count is K)
    _add('fwd-cols-N%d' % _N, fwd_case, B=33, K=64, N=_N)
    _add('bwd-cols-N%d' % _N, bwd_case, B=33, K=64, N=_N)
    _add('dinput-cols-K%d' % _N, dinput_case, B=33, N=64, K=_N)
for _B in FORM_B:     # reduction edges, N = 33 (in the backward: the dW shapes)
    for _K, _ld, _K2 in RED:
        _add('fwd-red-B%d-K%d-ld%d-K2_%d' % (_B, _K, _ld, _K2), fwd_case, B=_B, K=_K, N=33, ld_in=_ld, K2=_K2)
        _add('bwd-red-B%d-K%d-ld%d-K2_%d' % (_B, _K, _ld, _K2), bwd_case, B=_B, K=_K, N=33, ld_in=_ld, K2=_K2)
    for _n in WT_RED:
        _add('dinput-red-B%d-N%d' % (_B, _n), dinput_case, B=_B, N=_n, K=33)
        _add('bwd-next-B%d-Nn%d' % (_B, _n), bwd_case, B=_B, K=64, N=33, src='next', N_next=_n)
_F = dict(K=60, K2=10, N=67)
for _B in FORM_B:     # forms: K = 60, K2 = 10, N = 67, ld_out = 72
    _f = dict(_F, B=_B, ld_out=72)
    _add('fwd-form-B%d-plain' % _B, fwd_case, bn=None, act=None, bias=False, save_y=False, **_f)
    _add('fwd-form-B%d-bias-add' % _B, fwd_case, bn=None, act=None, add=(3, 5), **_f)
    _add('fwd-form-B%d-bn-relu' % _B, fwd_case, **_f)
    _add('fwd-form-B%d-bn-leaky-drop' % _B, fwd_case, act='leaky_relu', drop=True, **_f)
    _add('fwd-form-B%d-bn-tanh' % _B, fwd_case, act='tanh', **_f)
    _add('fwd-form-B%d-bn-eval' % _B, fwd_case, bn='eval', **_f)
    _add('fwd-form-B%d-ema-biased' % _B, fwd_case, unbiased=0, **_f)
    _add('fwd-form-B%d-identity-bn' % _B, fwd_case, B=_B, K=67, N=67, ld_in=72, ld_out=72, identity=True, bias=False)
    _add('fwd-form-B%d-identity-drop' % _B, fwd_case, B=_B, K=67, N=67, ld_in=72, ld_out=72, identity=True, bias=False, bn=None, act=None, drop=True,
         save_y=False)
    _g = dict(_F, B=_B)
    _add('bwd-form-B%d-dout-bn-relu-drop' % _B, bwd_case, ld_dout=72, drop=True, **_g)
    _add('bwd-form-B%d-next-bn-leaky' % _B, bwd_case, src='next', act='leaky_relu', **_g)
    _add('bwd-form-B%d-dout-bn-tanh' % _B, bwd_case, ld_dout=72, act='tanh', **_g)
    _add('bwd-form-B%d-dout-frozen-relu' % _B, bwd_case, ld_dout=72, bn='frozen', **_g)
    _add('bwd-form-B%d-next-frozen-leaky-drop' % _B, bwd_case, src='next', bn='frozen', act='leaky_relu', drop=True, **_g)
    _add('bwd-form-B%d-dout-nobn-none' % _B, bwd_case, ld_dout=72, bn=None, act=None, **_g)
    _add('bwd-form-B%d-next-nobn-relu-drop' % _B, bwd_case, src='next', bn=None, drop=True, **_g)
    _add('bwd-form-B%d-dout-nobn-leaky' % _B, bwd_case, ld_dout=72, bn=None, act='leaky_relu', **_g)
    _add('bwd-form-B%d-no-dw' % _B, bwd_case, ld_dout=72, dw=False, **_g)
    _add('bwd-form-B%d-no-dparams' % _B, bwd_case, ld_dout=72, dparams=False, **_g)
    _add('bwd-form-B%d-nobn-no-dbias' % _B, bwd_case, src='next', bn=None, dparams=False, **_g)
    for _al in (1.0, -1.0, 0.5):
        _add('dinput-form-B%d-alpha%g' % (_B, _al), dinput_case, B=_B, N=67, K=60, alpha=_al)
    _add('dinput-form-B%d-add-strided' % _B, dinput_case, B=_B, N=67, K=60, alpha=-1.0, ld_add=63, ld_din=63)
for _B in FUSED_B:    # the fused pooled batch-norm backward of t3d_fc_dinput
    for _K in FUSED_K:
        _add('dinput-fused-B%d-K%d-train' % (_B, _K), dinput_case, B=_B, N=64, K=_K, fused='train')
        _add('dinput-fused-B%d-K%d-frozen' % (_B, _K), dinput_case, B=_B, N=64, K=_K, fused='frozen')
        _add('dinput-fused-B%d-K%d-no-dparams' % (_B, _K), dinput_case, B=_B, N=64, K=_K, fused='train', dparams=False)

CASE_IDS = list(CASES)
RIDER_IDS = [c for c in CASE_IDS if CASES[c][1]['B'] <= 32]                  # part 2: the rider form takes B <= 32
PAIRED_IDS = [c for c in CASE_IDS if not c.startswith('fwd')]                # t3d_small_pair takes fc_bwd and fc_dinput
LONG_RIDER_IDS = ['fwd-red-B31-K1096-ld1096-K2_0', 'bwd-red-B31-K1096-ld1096-K2_0']      # K > 384: a second GIF = 6 batch; Kt > 256: the looped dW behind XKB = 2
assert all(c in RIDER_IDS for c in LONG_RIDER_IDS)


def make(cid):
    f, kw = CASES[cid]
    return f(**kw)


def check_case(env, cid, stats=None):
    """One stand-alone launch against the fp64 specification (ORACLE_TOL; padding columns keep the sentinel), guard bands."""
    case = make(cid)
    check_against_oracle(env, SPEC, case, cid, verbose=stats is not None, stats=stats)
    check_guards(run_apart(env, case, reps=1), cid + ' stand-alone')


def check_rider(env, cid):
    """Part 2: the op as a one-op rider set through t3d_run_riders against its stand-alone launch, bit for bit, REPS repetitions."""
    check_set_alone(env, make(cid), what=cid)


def check_margins(cid):
    case = make(cid)
    f = getattr(case, 'facts', None)
    if f is None or f['act'] not in ('relu', 'leaky_relu'):
        return 0
    bad = margin_violations(f['y'], f['mean'], f['invstd'], f['gamma'], f['beta'], f['bn'])
    assert not bad.any(), '%s: %d elements of z within %d fp32 spacings of 0' % (cid, int(bad.sum()), MARGIN_ULPS)
    return 1


# ---- the K = 1096 reduction in float32 ------------------------------------------------------------------------------------------------------------
def check_long_reduction_in_float32(B):
    """The K = 1096 forward (longer than any existing FC case) with a float32 accumulator in NumPy -- one running sum over all 1096
    terms, a longer chain than any of the kernel's (eight waves' partial sums) -- against the fp64 specification: the error must use less
    than a quarter of ORACLE_TOL['fc_fwd'] before the bound is relied on."""
    case = make('fwd-red-B%d-K1096-ld1096-K2_0' % B)
    b = Bufs(SPEC.dev)
    (_, a), = case(b)
    x, w = arr(a.in_, B, a.ld_in)[:, :a.K].copy(), arr(a.w, a.K, a.N).copy()
    bias, gamma, beta = arr(a.bias, a.N).copy(), arr(a.gamma, a.N).copy(), arr(a.beta, a.N).copy()
    rc.call_op(SPEC, 't3d_fc_fwd', a)
    ref = arr(a.out, B, a.ld_out)[:, :a.N].astype(np.float64)
    acc = np.zeros((B, a.N), np.float32)
    for k in range(a.K):
        acc = acc + x[:, k:k + 1] * w[k:k + 1]
    y = acc + bias
    mean = y.mean(0, dtype=np.float32)
    var = ((y - mean) ** 2).mean(0, dtype=np.float32)
    out = np.maximum((y - mean) * (np.float32(1) / np.sqrt(var + np.float32(EPS))) * gamma + beta, 0)
    assert out.dtype == np.float32
    rtol, atol, _ = rc.ORACLE_TOL['fc_fwd']('out')
    ratio = float((np.abs(out - ref) / (atol + rtol * np.abs(ref))).max())
    assert ratio < 0.25, ratio
    return ratio


# ---- refusals of the three stand-alone launchers -----------------------------------------------------------------------------------------------------
def _null(*fields):
    def m(a, b):
        for f in fields:
            setattr(a, f, None)
    return m


def _set(**kw):
    def m(a, b):
        for k, v in kw.items():
            setattr(a, k, v)
    return m


def _with_in2(**kw):
    def m(a, b):
        a.in2, a.ld_in2 = fptr(b.inp(np.zeros((a.B, 4), np.float32))), 4
        for k, v in kw.items():
            setattr(a, k, v)
    return m


_FW = dict(B=8, K=16, N=16, K2=4)
_FWI = dict(B=8, K=16, N=16, identity=True, bias=False)
_BW = dict(B=8, K=16, N=16, K2=4)
_BWN = dict(B=8, K=16, N=16, src='next', N_next=8)
_DI = dict(B=8, N=16, K=16, fused='train')
# every `return T3D_ERR_*` of csrc/fc.hip (t3d_fc_fwd) and csrc/fc_dev.h (check_fc_bwd, check_fc_dinput): (id, factory, kwargs, mutation, code)
REFUSALS = (
    [('fwd-' + n, fwd_case, kw, m, c) for n, kw, m, c in [
        ('in', _FW, _null('in_'), ERR_ARG), ('out', _FW, _null('out'), ERR_ARG), ('in2', _FW, _null('in2'), ERR_ARG),
        ('identity-K', _FWI, _set(K=15), ERR_SHAPE), ('identity-K2', _FWI, _with_in2(K2=4), ERR_SHAPE),
        ('beta', _FW, _null('beta'), ERR_ARG), ('moving_mean', _FW, _null('moving_mean'), ERR_ARG), ('moving_var', _FW, _null('moving_var'), ERR_ARG),
        ('mean', _FW, _null('mean'), ERR_ARG), ('invstd', _FW, _null('invstd'), ERR_ARG), ('y', _FW, _null('y'), ERR_ARG),
        ('decay', _FW, _null('decay'), ERR_ARG), ('B0', _FW, _set(B=0), ERR_SHAPE), ('B129', _FW, _set(B=129), ERR_SHAPE),
        ('N0', _FW, _set(N=0), ERR_SHAPE), ('K0', _FW, _set(K=0), ERR_SHAPE)]] +
    [('bwd-' + n, bwd_case, kw, m, c) for n, kw, m, c in [
        ('dy', _BW, _null('dy'), ERR_ARG), ('dout', _BW, _null('dout'), ERR_ARG), ('dy_next', _BWN, _null('dy_next'), ERR_ARG),
        ('w_next', _BWN, _null('w_next'), ERR_ARG), ('in', _BW, _null('in_'), ERR_ARG), ('in2', _BW, _null('in2'), ERR_ARG),
        ('beta', _BW, _null('beta'), ERR_ARG), ('mean', _BW, _null('mean'), ERR_ARG), ('invstd', _BW, _null('invstd'), ERR_ARG),
        ('y', _BW, _null('y'), ERR_ARG), ('act-y', dict(_BW, bn=None), _null('y'), ERR_ARG),
        ('B0', _BW, _set(B=0), ERR_SHAPE), ('B129', _BW, _set(B=129), ERR_SHAPE), ('N0', _BW, _set(N=0), ERR_SHAPE)]] +
    [('dinput-' + n, dinput_case, _DI, m, c) for n, m, c in [
        ('dy', _null('dy'), ERR_ARG), ('w', _null('w'), ERR_ARG), ('din', _null('din'), ERR_ARG),
        ('bn_pooled', _null('bn_pooled'), ERR_ARG), ('bn_ysel', _null('bn_ysel'), ERR_ARG), ('bn_dpool', _null('bn_dpool'), ERR_ARG),
        ('bn_scale', _null('bn_scale'), ERR_ARG), ('bn_gamma', _null('bn_gamma'), ERR_ARG), ('bn_mean', _null('bn_mean'), ERR_ARG),
        ('bn_invstd', _null('bn_invstd'), ERR_ARG), ('B0', _set(B=0), ERR_SHAPE), ('B129', _set(B=129), ERR_SHAPE),
        ('N0', _set(N=0), ERR_SHAPE), ('K0', _set(K=0), ERR_SHAPE)]])
REFUSAL_IDS = [r[0] for r in REFUSALS]


def _refused(env, b, call, want, what):
    before = b.snapshot()
    for lib_env in (env, SPEC) if env is not SPEC else (SPEC,):
        got = call(lib_env)
        assert got == want, '%s: %s answered %d, expected %d' % (what, type(lib_env.lib).__name__, got, want)
    env.sync()
    assert_same_bits(before, b.snapshot(), what + ': a refused call wrote')


def check_refusal(env, rid):
    """The launcher and the specification answer the same code, and nothing was written.  (The specification gets the same struct: a
    refusal touches no pointer, so device pointers do no harm there.)"""
    _, factory, kw, mutate, want = REFUSALS[REFUSAL_IDS.index(rid)]
    b = Bufs(env.dev)
    (name, a), = factory(**kw)(b)
    assert getattr(env.lib, name)(C.byref(a), env.stream()) == 0, rid + ': the case is refused before its mutation'      # the case is valid
    env.sync()
    b2 = Bufs(env.dev)
    (name, a), = factory(**kw)(b2)
    mutate(a, b2)
    _refused(env, b2, lambda e: getattr(e.lib, name)(C.byref(a), e.stream()), want, rid)


def check_null_struct(env):
    for name in ('t3d_fc_fwd', 't3d_fc_bwd', 't3d_fc_dinput'):
        for e in (env, SPEC):
            assert getattr(e.lib, name)(None, e.stream()) == ERR_ARG, name


# ---- part 3: t3d_small_pair ------------------------------------------------------------------------------------------------------------------------
def pair_case(fa, fb):
    def case(b):
        return fa(_Tag(b, 'a.')) + fb(_Tag(b, 'b.'))
    return case


def run_pair(env, case, reps=REPS):
    b = Bufs(env.dev)
    (n1, a1), (n2, a2) = case(b)
    o1, o2 = small_op(n1, a1), small_op(n2, a2)
    for _ in range(reps):
        got = env.lib.t3d_small_pair(C.byref(o1), C.byref(o2), env.stream())
        assert got == 0, ('t3d_small_pair', got)
    env.sync()
    return b.snapshot()


def check_pair(env, case, what, stats=None):
    """The pair against the two stand-alone launches on fresh buffers, bit for bit (guard bands included, REPS repetitions); and ONE
    paired launch against the specification's t3d_small_pair with ORACLE_TOL."""
    ref, got = run_apart(env, case), run_pair(env, case)
    check_guards(ref, what + ' stand-alone')
    check_guards(got, what + ' paired')
    assert_same_bits(ref, got, what + ': paired vs stand-alone launches')
    bc = Bufs(SPEC.dev)
    ops = case(bc)
    init = bc.snapshot()
    once, spec = run_pair(env, case, reps=1), None
    assert SPEC.lib.t3d_small_pair(C.byref(small_op(*ops[0])), C.byref(small_op(*ops[1])), None) == 0
    spec = bc.snapshot()
    for k in once:
        if (once[k][0] == init[k][0]).all():
            continue                                     # (dgamma / dbeta of a frozen fc_bwd: left alone by both)
        name, a = ops[0] if k.startswith('a.') else ops[1]
        kind = rc.ORACLE_KIND[name]
        rc.compare_with_spec(once, spec, k, kind, kind == 'fc_dinput' and bool(a.bn_pooled), what + ' paired', stats is not None, stats)


def _p_bn(dense, N=16, T=8, seed=2):
    return lambda: rc.bn_bwd_case(N, T, dense, seed=seed)


_SMALL = {      # one small op of each kind, in two variants (a pair of one kind takes one of each)
    'bn_bwd': (_p_bn(True), _p_bn(False, N=33, seed=5)),
    'fc_bwd': (lambda: bwd_case(B=31, K=60, K2=10, N=67, ld_dout=72, drop=True), lambda: bwd_case(B=2, K=13, N=33, src='next', N_next=9, bn=None)),
    'fc_dinput': (lambda: dinput_case(B=31, N=67, K=60, alpha=-1.0, ld_add=63, ld_din=63), lambda: dinput_case(B=1, N=64, K=33, fused='train')),
    'dy_colsum': (lambda: rc.dy_colsum_case(2, 128), lambda: rc.dy_colsum_case(3, 67, tpf=3, seed=9)),
}
_KINDS = ['bn_bwd', 'fc_bwd', 'fc_dinput', 'dy_colsum']
PAIRS = {}
for _a in _KINDS:      # every ordered pair of the four kinds, k_small_pair<1>
    for _b in _KINDS:
        PAIRS['%s+%s' % (_a, _b)] = (_SMALL[_a][0], _SMALL[_b][1])
_BIG = {'fc_bwd-B33': lambda: bwd_case(B=33, K=60, K2=10, N=67, ld_dout=72, drop=True), 'fc_dinput-B128': lambda: dinput_case(B=128, N=67, K=96, fused='train'),
        'fc_bwd-B128': lambda: bwd_case(B=128, K=72, N=33, src='next', N_next=100, act='leaky_relu'), 'fc_dinput-B33': lambda: dinput_case(B=33, N=100, K=67, ld_din=72)}
_PARTNER = {'bn_bwd-dense-T8': _p_bn(True), 'bn_bwd-dense-T512': _p_bn(True, N=33, T=512), 'bn_bwd-pooled': _p_bn(False, N=33, seed=5),
            'dy_colsum': lambda: rc.dy_colsum_case(2, 128), 'fc_bwd-B97': lambda: bwd_case(B=97, K=13, N=33, bn=None, act='leaky_relu'),
            'fc_dinput-B97': lambda: dinput_case(B=97, N=9, K=33)}
for _i, (_f, _ff) in enumerate(_BIG.items()):      # k_small_pair<MAXRB>: an FC op of more than 32 rows beside each partner, orders alternating
    for _j, (_q, _qf) in enumerate(_PARTNER.items()):
        if (_i + _j) % 2 == 0:
            PAIRS['%s+%s' % (_f, _q)] = (_ff, _qf)
        else:
            PAIRS['%s+%s' % (_q, _f)] = (_qf, _ff)
_W1 = lambda: bwd_case(B=31, K=8, N=1, bn=None, act=None)                       # 1 block
_W64 = lambda: dinput_case(B=31, N=8, K=2048)                                   # 64 blocks
_V1 = lambda: dinput_case(B=31, N=8, K=1)
_V64 = lambda: bwd_case(B=31, K=8, N=2048)
_R67a = lambda: bwd_case(B=31, K=60, K2=10, N=67, src='next', N_next=9)         # 3 blocks, the last ragged
_R67b = lambda: dinput_case(B=31, N=100, K=67, ld_din=72)
for _n, _fa, _fb in [('bwd-N1+dinput-K2048', _W1, _W64), ('dinput-K2048+bwd-N1', _W64, _W1), ('dinput-K1+bwd-N2048', _V1, _V64),
                     ('bwd-N2048+dinput-K1', _V64, _V1), ('bwd-N67+dinput-K67', _R67a, _R67b), ('dinput-K67+bwd-N67', _R67b, _R67a),
                     ('bwd-N67+dinput-K2048', _R67a, _W64), ('bwd-N2048+dinput-K67', _V64, _R67b)]:
    PAIRS['blocks-' + _n] = (_fa, _fb)
PAIRS['bn_bwd-frozen-null-stats+fc_bwd'] = (lambda: bn_bwd_frozen_case(33, False), _SMALL['fc_bwd'][0])
PAIRS['fc_dinput+bn_bwd-frozen-null-stats-dense'] = (_SMALL['fc_dinput'][0], lambda: bn_bwd_frozen_case(33, True))
PAIR_IDS = list(PAIRS)


def check_pair_id(env, pid, stats=None):
    fa, fb = PAIRS[pid]
    check_pair(env, pair_case(fa(), fb()), pid, stats)


def check_case_in_a_pair(env, cid):
    """A part-1 case beside a small partner (dy_colsum or a finalizer, before or behind it by the case's position in the table): the
    ragged shapes through k_small_pair<1> / <MAXRB>, bit for bit against the stand-alone launches."""
    i = PAIRED_IDS.index(cid)
    partner = rc.dy_colsum_case(2, 128) if i % 4 < 2 else rc.bn_bwd_case(16, 8, True)
    case = pair_case(make(cid), partner) if i % 2 == 0 else pair_case(partner, make(cid))
    ref, got = run_apart(env, case, reps=1), run_pair(env, case, reps=1)
    check_guards(got, cid + ' paired')
    assert_same_bits(ref, got, cid + ': paired vs stand-alone launches')


def check_bn_bwd_frozen(env, dense, stats=None):
    """t3d_bn_bwd_finalize, frozen, gamma = mean = invstd = NULL: stand-alone against the specification, and as a one-op rider set."""
    case = bn_bwd_frozen_case(33, dense)
    check_against_oracle(env, SPEC, case, 'bn_bwd frozen dense=%d' % dense, verbose=stats is not None, stats=stats)
    check_set_alone(env, case, what='bn_bwd frozen dense=%d' % dense)


def _kind(k):
    def m(o1, o2, b):
        o1.kind = k
    return m


def _u(which, field, **kw):
    def m(o1, o2, b):
        u = getattr((o1, o2)[which].u, field)
        for k, v in kw.items():
            setattr(u, k, v)
    return m


_PB, _PD, _PN, _PC = _SMALL['fc_bwd'][0], _SMALL['fc_dinput'][0], _p_bn(True), _SMALL['dy_colsum'][0]
PAIR_REFUSALS = [      # (id, a, b, mutation of the two t3d_small_op, code)
    ('a-null', _PB, _PC, 'a', ERR_ARG), ('b-null', _PB, _PC, 'b', ERR_ARG)] + [
    ('kind-%d' % k, _PB, _PC, _kind(k), ERR_ARG) for k in (0, 5, 6, 7, 8)] + [
    ('kind-b-6', _PC, _PB, lambda o1, o2, b: setattr(o2, 'kind', 6), ERR_ARG),
    ('bn_bwd-coef', _PN, _PC, _u(0, 'bn_bwd', coef=None), ERR_ARG),
    ('bn_bwd-T513', _PC, _PN, _u(1, 'bn_bwd', n_tiles=513), ERR_ARG),
    ('bn_bwd-gamma', _PN, _PC, _u(0, 'bn_bwd', gamma=None), ERR_ARG),
    ('fc_bwd-dy', _PB, _PC, _u(0, 'fc_bwd', dy=None), ERR_ARG),
    ('fc_bwd-dout', _PC, _PB, _u(1, 'fc_bwd', dout=None), ERR_ARG),
    ('fc_bwd-y', _PB, _PD, _u(0, 'fc_bwd', y=None), ERR_ARG),
    ('fc_dinput-w', _PB, _PD, _u(1, 'fc_dinput', w=None), ERR_ARG),
    ('dy_colsum-out', _PB, _PC, _u(1, 'dy_colsum', out=None), ERR_ARG),
    ('rows-32+33', lambda: bwd_case(B=32, K=16, N=16), lambda: dinput_case(B=33, N=16, K=16), None, ERR_SHAPE),
    ('rows-33+32', lambda: dinput_case(B=33, N=16, K=16), lambda: bwd_case(B=32, K=16, N=16), None, ERR_SHAPE),
    ('B129', _PB, _PC, _u(0, 'fc_bwd', B=129), ERR_SHAPE), ('B129-dinput', _PC, _PD, _u(1, 'fc_dinput', B=129), ERR_SHAPE),
    ('B0', _PB, _PC, _u(0, 'fc_bwd', B=0), ERR_SHAPE)]
PAIR_REFUSAL_IDS = [r[0] for r in PAIR_REFUSALS]


def check_pair_refusal(env, rid):
    _, fa, fb, mutate, want = PAIR_REFUSALS[PAIR_REFUSAL_IDS.index(rid)]
    b = Bufs(env.dev)
    (n1, a1), (n2, a2) = pair_case(fa(), fb())(b)
    o1, o2 = small_op(n1, a1), small_op(n2, a2)
    p1, p2 = C.byref(o1), C.byref(o2)
    if mutate == 'a':
        p1 = None
    elif mutate == 'b':
        p2 = None
    elif mutate is not None:
        mutate(o1, o2, b)
    _refused(env, b, lambda e: e.lib.t3d_small_pair(p1, p2, e.stream()), want, 'pair ' + rid)


# ---- the tests must be able to fail: deliberately wrong specifications -------------------------------------------------------------------------------
def _copy(p):
    q = type(p)()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


class StatsOverPaddedRows(FakeLib):
    """batch statistics over 32 ceil(B / 32) rows (the rows past B as zeros)"""
    @staticmethod
    def _fc_stats(y):
        yp = np.concatenate([y, np.zeros(((-len(y)) % 32, y.shape[1]))], 0)
        return FakeLib._fc_stats(yp)


class LastColumnDropped(FakeLib):
    def t3d_fc_fwd(self, a, stream):
        got = super().t3d_fc_fwd(a, stream)
        p = a._obj
        arr(p.out, p.B, p.ld_out)[:, p.N - 1] = 0
        return got


class In2IgnoredInStraddle(FakeLib):
    """the elements of in2 that share a k-group of 8 with the end of `in` read as 0"""
    @staticmethod
    def _fc_in(p):
        x = FakeLib._fc_in(p)
        if p.K2 > 0 and p.K % 8:
            x[:, p.K:min(p.K + p.K2, (p.K + 7) // 8 * 8)] = 0
        return x


class ReductionTailDropped(FakeLib):
    """the last Kt mod 8 reduction elements dropped"""
    @staticmethod
    def _fc_in(p):
        x = FakeLib._fc_in(p)
        Kt = p.K + p.K2
        x[:, Kt - Kt % 8:] = 0
        return x


class BiasedEma(FakeLib):
    def t3d_fc_fwd(self, a, stream):
        q = _copy(a._obj)
        q.unbiased_ema = 0
        return super().t3d_fc_fwd(C.byref(q), stream)


class PaddingColumnWritten(FakeLib):
    def t3d_fc_fwd(self, a, stream):
        got = super().t3d_fc_fwd(a, stream)
        p = a._obj
        if p.ld_out > p.N:
            arr(p.out, p.B, p.ld_out)[:, p.ld_out - 1] = 0
        return got


class DwTailRowsDropped(FakeLib):
    """dW rows >= 32 floor(Kt / 32) dropped"""
    def t3d_fc_bwd(self, a, stream):
        got = super().t3d_fc_bwd(a, stream)
        p = a._obj
        if p.dw:
            Kt = p.K + p.K2
            arr(p.dw, Kt, p.N)[Kt // 32 * 32:] = 0
        return got


class WNextWrongStride(FakeLib):
    """w_next read with ldw = N_next + 1"""
    @staticmethod
    def _w_next(p):
        flat = arr(p.w_next, p.N * p.N_next)
        idx = np.arange(p.N)[:, None] * (p.N_next + 1) + np.arange(p.N_next)[None]
        return flat[np.minimum(idx, flat.size - 1)].astype(np.float64)


# mutant -> (cases that must catch it, cases of the same table that must not: the shapes the mutation does not reach)
MUTANTS = {
    StatsOverPaddedRows: (['fwd-rows-B33', 'fwd-rows-B1', 'fwd-rows-B97', 'fwd-cols-N67'], ['fwd-rows-B32', 'fwd-rows-B128']),
    LastColumnDropped: (['fwd-cols-N1', 'fwd-cols-N33', 'fwd-cols-N67', 'fwd-rows-B33'], []),
    In2IgnoredInStraddle: (['fwd-red-B31-K60-ld60-K2_10', 'bwd-red-B97-K60-ld60-K2_10', 'fwd-form-B97-bn-relu'], ['fwd-red-B31-K64-ld68-K2_10']),
    ReductionTailDropped: (['fwd-red-B31-K3-ld3-K2_0', 'fwd-red-B97-K13-ld13-K2_0', 'fwd-red-B31-K60-ld60-K2_0', 'fwd-red-B31-K60-ld60-K2_10',
                            'fwd-red-B97-K68-ld70-K2_0', 'bwd-red-B31-K60-ld60-K2_0'], ['fwd-red-B31-K72-ld72-K2_0', 'fwd-red-B31-K1096-ld1096-K2_0']),
    BiasedEma: (['fwd-rows-B2', 'fwd-rows-B33', 'fwd-form-B31-bn-relu'], ['fwd-form-B31-ema-biased', 'fwd-rows-B1']),
    PaddingColumnWritten: (['fwd-rows-B33', 'fwd-form-B31-plain', 'fwd-form-B97-identity-bn'], ['fwd-cols-N33']),
    DwTailRowsDropped: (['bwd-red-B31-K60-ld60-K2_0', 'bwd-red-B97-K3-ld3-K2_0', 'bwd-red-B31-K1096-ld1096-K2_0', 'bwd-form-B97-dout-bn-tanh'],
                        ['bwd-rows-B33', 'bwd-cols-N67']),
    WNextWrongStride: (['bwd-next-B31-Nn3', 'bwd-next-B97-Nn9', 'bwd-next-B31-Nn96', 'bwd-form-B31-next-bn-leaky'], ['bwd-rows-B33']),
}


def caught(mutant_cls, cid):
    """does the part-1 check of case `cid` fail on the deliberately wrong library?"""
    try:
        check_against_oracle(Env(mutant_cls(), 'cpu'), SPEC, make(cid), cid, verbose=False)
    except AssertionError:
        return True
    return False


# ---- the specification itself against autograd ------------------------------------------------------------------------------------------------------------
AUTOGRAD_FORMS = ['nobn-bias', 'bn-relu-drop', 'bn-leaky', 'bn-tanh', 'eval-relu', 'nobn-relu-add']


def check_spec_against_autograd(form, B=13, K=11, K2=5, N=9):
    """One FC layer of each form in fp64 torch, differentiated by autograd, against the y, out, dy, dW, dbias, dgamma, dbeta and din the
    specification returns (which stores y and dy as fp32: 1e-5).  Under eval-mode batch-norm the layer's dbias / dgamma / dbeta are left
    out: t3d.h says t3d_fc_bwd does not compute them with bn_training == 0."""
    import torch
    bn = None if form.startswith('nobn') else ('eval' if form.startswith('eval') else 'train')
    act = {'nobn-bias': None, 'bn-relu-drop': 'relu', 'bn-leaky': 'leaky_relu', 'bn-tanh': 'tanh', 'eval-relu': 'relu', 'nobn-relu-add': 'relu'}[form]
    drop, add = form == 'bn-relu-drop', ((3, 5) if form == 'nobn-relu-add' else None)
    b = Bufs(SPEC.dev)
    (_, f), = fwd_case(B, K, N, ld_in=K + 2, K2=K2, ld_out=N + 3, bn=bn, act=act, drop=drop, add=add)(b)
    x = np.concatenate([arr(f.in_, B, f.ld_in)[:, :K], arr(f.in2, B, f.ld_in2)[:, :K2]], 1).astype(np.float64)
    mm0, mv0 = (arr(f.moving_mean, N).copy(), arr(f.moving_var, N).copy()) if bn else (None, None)
    assert SPEC.lib.t3d_fc_fwd(C.byref(f), None) == 0
    t = lambda v, g=True: torch.tensor(np.asarray(v, np.float64), requires_grad=g)
    xt, wt, bt = t(x), t(arr(f.w, K + K2, N)), t(arr(f.bias, N))
    yt = xt @ wt + bt
    yt.retain_grad()
    z = yt
    if bn:
        gt, bet = t(arr(f.gamma, N)), t(arr(f.beta, N))
        mean, var = (yt.mean(0), yt.var(0, unbiased=False)) if bn == 'train' else (t(mm0, False), t(mv0, False))
        z = (yt - mean) / torch.sqrt(var + EPS) * gt + bet
    z = {None: lambda v: v, 'relu': torch.relu, 'leaky_relu': lambda v: torch.nn.functional.leaky_relu(v, ALPHA), 'tanh': torch.tanh}[act](z)
    if drop:
        z = z * t(arr(f.drop_mask, B, N), False) / KEEP
    if add:
        z = torch.cat([z[:, :3] + t(arr(f.add_in, B, 5)[:, :3], False), z[:, 3:]], 1)
    G = np.random.RandomState(5).normal(size=(B, N)).astype(np.float32).astype(np.float64)      # (exactly what the fp32 dout holds)
    (z * t(G, False)).sum().backward()
    close = lambda got, ref, what: np.testing.assert_allclose(got, ref.detach().numpy(), rtol=1e-5, atol=1e-5, err_msg=form + ' ' + what)
    close(arr(f.y, B, N), yt, 'y')
    close(arr(f.out, B, f.ld_out)[:, :N], z, 'out')
    if bn == 'train':
        np.testing.assert_allclose(arr(f.moving_var, N), mv0 * DECAY + yt.var(0, unbiased=True).detach().numpy() * (1 - DECAY), rtol=1e-5, err_msg='moving_var')
    # backward: the saved activations are the forward's
    g = abi.FcBwdArgs()
    dout = b.inp(G.astype(np.float32))
    g.dout, g.ld_dout = fptr(dout), N
    g.in_, g.ld_in, g.K, g.in2, g.ld_in2, g.K2 = f.in_, f.ld_in, K, f.in2, f.ld_in2, K2
    g.y, g.gamma, g.beta, g.mean, g.invstd = f.y, f.gamma, f.beta, f.mean, f.invstd
    g.bn_training, g.act, g.leaky_alpha, g.drop_mask, g.keep_prob = int(bn == 'train'), f.act, ALPHA, f.drop_mask, KEEP
    dy, dw, db, dg, dbe = (b.out(k, s) for k, s in (('dy', (B, N)), ('dw', (K + K2, N)), ('db', N), ('dg', N), ('dbe', N)))
    g.dy, g.dw, g.dbias, g.dgamma, g.dbeta, g.B, g.N = fptr(dy), fptr(dw), fptr(db), fptr(dg), fptr(dbe), B, N
    assert SPEC.lib.t3d_fc_bwd(C.byref(g), None) == 0
    close(dy.numpy(), yt.grad, 'dy')
    close(dw.numpy(), wt.grad, 'dW')
    if bn != 'eval':
        close(db.numpy(), bt.grad, 'dbias')
    if bn == 'train':
        close(dg.numpy(), gt.grad, 'dgamma')
        close(dbe.numpy(), bet.grad, 'dbeta')
    d = abi.FcDinputArgs()
    din = b.out('din', (B, K + 1))
    wk = b.inp(arr(f.w, K + K2, N)[:K].copy())
    d.dy, d.N, d.w, d.alpha, d.din, d.ld_din, d.B, d.K = fptr(dy), N, fptr(wk), 1.0, fptr(din), K + 1, B, K
    assert SPEC.lib.t3d_fc_dinput(C.byref(d), None) == 0
    close(din.numpy()[:, :K], xt.grad[:, :K], 'din')


# ---- the tables of the GPU module's docstring ----------------------------------------------------------------------------------------------------------
FORMS = [
    ('RBT = 1 (B <= 32) / RBT = MAXRB (B > 32), stand-alone', 'test_fc_against_spec[*-rows-B1 .. B32], [*-rows-B33 .. B128]'),
    ('partly filled row blocks (B = 33, 65, 97, 127), B = 1 (variance 0)', 'test_fc_against_spec[*-rows-*]'),
    ('ragged last column block, one column, two blocks', 'test_fc_against_spec[*-cols-*]'),
    ('vector k-loop only (K % 8 == 0, ld_in % 4 == 0)', 'test_fc_against_spec[*-red-*-K8-*], [*-K72-*], [*-K1096-*], [*-rows-*]'),
    ('scalar k-loop only (ld_in & 3 != 0, or K < 8)', 'test_fc_against_spec[*-red-*-K3-*], [*-K13-*], [*-K68-ld70-*]'),
    ('`gfull` tail: vector groups, then a half group', 'test_fc_against_spec[*-red-*-K60-ld60-K2_0]'),
    ('a k-group straddling in | in2, ragged end at 70', 'test_fc_against_spec[*-red-*-K60-ld60-K2_10], [*-form-*]'),
    ('vector loop at a stride that is not K, scalar groups in in2', 'test_fc_against_spec[*-red-*-K64-ld68-K2_10]'),
    ('idle waves (1 group: seven; 9 groups: waves with 2, 1, 0)', 'test_fc_against_spec[*-red-*-K8-*], [*-K72-*]'),
    ('second GIF batch (RBT = 1: 16 groups per wave; MAXRB: 4; rider: 6)', 'test_fc_against_spec[*-red-B31-K1096-*], [*-red-B97-*], test_fc_rider_form[*-red-B31-K1096-*]'),
    ('prefetched dW (RBT = 1, blocks < 32) / looped dW (MAXRB; RBT = 1 beyond 32 blocks; rider beyond 8)',
     'test_fc_against_spec[bwd-*-B31-*], [bwd-*-B97-*], [bwd-red-B31-K1096-*], test_fc_rider_form[bwd-red-B31-K1096-*]'),
    ('dW store guard kk < Kt, at_nb through in2', 'test_fc_against_spec[bwd-red-*]'),
    ('wave_gemm<true> scalar (ldw = 3, 9, 67) / vector (96) / vector then half group (100)', 'test_fc_against_spec[dinput-red-*], [bwd-next-*]'),
    ('identity form (w == NULL)', 'test_fc_against_spec[fwd-form-*-identity-*]'),
    ('optional pointers, activations, dropout, add_in, eval / frozen batch-norm, unbiased_ema = 0', 'test_fc_against_spec[*-form-*]'),
    ('fused pooled batch-norm backward of fc_dinput: training, frozen with NULL statistics, no dgamma / dbeta', 'test_fc_against_spec[dinput-fused-*]'),
    ('rider form (256 threads, NWP = 4, GIF = 6, XKB = 2)', 'test_fc_rider_form'),
    ('paired form, k_small_pair<1>', 'test_fc_case_in_a_pair[*-B1 .. B32-*], test_small_pair[<kind>+<kind>], [blocks-*]'),
    ('paired form, k_small_pair<MAXRB>', 'test_fc_case_in_a_pair[*-B33 .. B128-*], test_small_pair[*-B33*], [*-B128*]'),
    ('k_small_pair without an FC op (rows = 0)', 'test_small_pair[dy_colsum+dy_colsum], [bn_bwd+bn_bwd], [bn_bwd+dy_colsum], [dy_colsum+bn_bwd]'),
    ('blockIdx.x < n_a split: 1 block beside 64, both orders; ragged N = 67 on both sides', 'test_small_pair[blocks-*]'),
    ('frozen bn_bwd_finalize with gamma = mean = invstd = NULL', 'test_bn_bwd_frozen_with_null_statistics, test_small_pair[*frozen-null-stats*]'),
    ('refusals of t3d_fc_fwd / t3d_fc_bwd / t3d_fc_dinput / t3d_small_pair', 'test_fc_refusals, test_fc_null_struct, test_small_pair_refusals'),
]


def forms_text():
    return 'FORM COVERAGE (mechanism -> test ids of this module)\n' + ''.join('  %-105s %s\n' % f for f in FORMS)


def stats_text(stats):
    return ''.join('  %-10s %-10s %.3e  (%.3e)  %.3f   %s\n' % (k[0], k[1], v[0], v[1], v[2], v[3]) for k, v in sorted(stats.items()))
