"""GPU: every dispatch variant of the point-MLP launchers (csrc/pointmlp.hip) with ALL operands inside guard bands
(tests/guard_bands.py), padded layouts (ldx > K, coff != 0) wherever act_ok allows them, and fp64 references formed with torch
on the device from the same (bf16-rounded, on the bf16 path) operands.  Two things the other kernel modules cannot see:

  * what a kernel touches outside its operands.  Inputs are surrounded by NaN (front band, back band, row padding, the columns
    K .. roundup4(K)-1, everything behind scale[roundup4(K)-1]); outputs by a sentinel that must survive bit for bit, while every
    element of the output itself must have been written.  Valid lengths are t3d.h's, not the kernels'.
  * the instantiations no kernel-level test launched: each case is the smallest shape that selects its variant, and the selecting
    predicate (read off the launchers) stands in the case's id or comment.  docs/EXPERIMENTS.md ("Guard-banded kernel tests") holds
    the kernel names a trace of this module showed.

Tolerances are the ones of tests/test_kernels_bf16_gpu.py (close_bf16, its psum / slab bounds) and of test_pointmlp_fwd / _dgrad /
_wgrad in tests/test_kernels_gpu.py (_close), imported, none new.  A per-slab bound is the slab-sum bound of the bf16 module
applied to the split's own rows_per_split-row GEMM.

K % 128 != 0 with a bf16 source (K = 192, 320): the weight-gradient launcher used to take 128-row k-tiles there (wgrad_tile off the
plan's split, t3d_wgrad_plan itself at large M) although ActLoaderT<false, bf16_t> neither clamps nor masks -- wgrad_body's
`sa.init(la, k0, tid)` fetches scale / shift at k0 + li and the stager x columns k0 .. k0 + 127, i.e. 64 elements past column K in
the last k-tile (the products land in accumulator rows >= K, which the `if (k < K)` store path drops, so no RESULT shows it: found by
reading).  wgrad_tile now falls back to 64-row k-tiles for such a source; test_wgrad_bf16 / test_fused_backward hold the shapes.

Pool arg indices with duplicated rows (test_pool_arg_indices_with_duplicated_rows): which of several bit-identical rows a form
reports is not asserted.  Observed on an MI355X: see docs/EXPERIMENTS.md, same section (every form reported the LOWEST row index
of the tied rows, for the maximum and the minimum alike)."""
import ctypes as C

import numpy as np
import pytest
import torch

from guard_bands import assert_clean, guarded, roundup4
from test_kernels_bf16_gpu import close_bf16, rb
from test_kernels_gpu import _close
from transferable3d_amd import abi
from transferable3d_amd.abi import fptr, iptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, F32T = torch.bfloat16, torch.float32
NAN = float('nan')


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Ops:
    """The guarded operands of one launch."""

    def __init__(self):
        self.checks = {}

    def inp(self, name, t, dtype=F32T, ld=None, col0=0):
        v, c = guarded(tuple(t.shape), dtype, DEV, ld=ld, col0=col0, fill=t, name=name)
        self.checks[name] = c
        return v

    def out(self, name, shape, dtype=F32T):
        v, c = guarded(shape, dtype, DEV, name=name)
        self.checks[name] = c
        return v

    def verify(self):
        """after the launch: inputs untouched, output bands intact, every output element written"""
        torch.cuda.synchronize()
        for c in self.checks.values():
            c(written=True)


def _tail_nan(t, n):
    return torch.cat([t, torch.full((n - t.numel(),), NAN)])


def _arith(monkeypatch, arith):
    if arith is not None:
        monkeypatch.setenv('T3D_X3', '1' if arith == 'x3' else '0')


def make_act(ops, g, M, K, kind, rpf, bn, sub=False, padded=True, coff=None, x=None, name='x'):
    """kind: 'bf16' (coff 8, ldx K + 24), 'f32' (coff 4, ldx K + 12), 'raw' (ldx 8, coff 0 or 4); padded=False: ldx = K, coff = 0.
    Only columns coff .. coff + K - 1 are finite.  scale / shift: roundup4(K) floats, NaN from K on and behind; sub: [B, 4] with
    three valid columns.  Returns (ActSrc, the fp64 activation [M, K])."""
    bf = kind == 'bf16'
    if kind == 'raw':
        ldx, coff = 8, (0 if coff is None else coff)
    elif not padded:
        ldx, coff = (K if K > 4 else 4), 0
    else:
        ldx, coff = (K + 24, 8) if bf else (K + 12, 4)
    if x is None:
        x = torch.randn(M, K, generator=g)
    xv = ops.inp(name, x, BF if bf else F32T, ld=ldx, col0=coff)
    a = ops.checks[name].valid.double()
    sc = sh = sb = None
    if bn:
        s_, h_ = 0.5 + torch.rand(K, generator=g), torch.randn(K, generator=g) * 0.2
        if not bf:
            s_[::3] *= -1
        sc, sh = ops.inp(name + '.scale', _tail_nan(s_, roundup4(K))), ops.inp(name + '.shift', _tail_nan(h_, roundup4(K)))
        a = torch.relu(a * s_.double().to(DEV) + h_.double().to(DEV))
    if sub:
        s3 = torch.randn(M // rpf, 3, generator=g)
        sb = ops.inp(name + '.sub', s3, ld=4)
        a = a - s3.double().to(DEV).repeat_interleave(rpf, 0)[:, :K]
    return abi.ActSrc(fptr(xv), ldx, coff, fptr(sc), fptr(sh), int(bn), fptr(sb), 4, abi.BF16 if bf else abi.F32), a


def make_dy(ops, g, M, N, bf, rpf=None, pooled=False):
    """dense: dz, y [M, N], coef [3, N]; pooled-sparse (fp32): argidx, dpool [B, N].  Returns (DySrc, fp64 dy [M, N])."""
    dt = BF if bf else F32T
    y = torch.randn(M, N, generator=g)
    coef = torch.randn(3, N, generator=g)
    coef[2] *= 1e-3
    yv, cv = ops.inp('y', y, dt), ops.inp('coef', coef)
    c = coef.double().to(DEV)
    if pooled:
        B = M // rpf
        arg = torch.randint(-1, rpf, (B, N), generator=g, dtype=torch.int32)
        dp = torch.randn(B, N, generator=g)
        av, dv = ops.inp('argidx', arg, torch.int32), ops.inp('dpool', dp)
        rin = (torch.arange(M) % rpf)[:, None]
        dz = torch.where(arg.repeat_interleave(rpf, 0) == rin, dp.repeat_interleave(rpf, 0), torch.zeros(M, N)).double().to(DEV)
        src = abi.DySrc(fptr(None), fptr(yv), fptr(cv), iptr(av), fptr(dv), abi.F32)
    else:
        zv = ops.inp('dz', torch.randn(M, N, generator=g) * 1e-2, dt)
        dz = zv.double()
        src = abi.DySrc(fptr(zv), fptr(yv), fptr(cv), iptr(None), fptr(None), abi.BF16 if bf else abi.F32)
    dy = c[0] * dz + c[1] * yv.double() + c[2]
    return src, (rb(dy) if bf else dy)


def _sums_close_bf16(got, ref, absmax, what, rel=1e-4, eps=1.0):
    """the psum bound of tests/test_kernels_bf16_gpu.py"""
    err = float((got.double() - ref).abs().max())
    assert err < rel * (absmax + eps), (what, err, absmax)


# ================================================================================================ forward
def run_fwd(lib, M, K, N, rpf, bf, kind, *, bn=None, sub=False, rowbias=False, pool=False, mask=False, store_y=True, coff=None,
            padded=True, x=None, seed=0):
    g = torch.Generator(device='cpu').manual_seed(1000 * seed + M + K + N)
    B, T = M // rpf, M // 128
    bn = (K > 4) if bn is None else bn
    ops = Ops()
    src, act = make_act(ops, g, M, K, kind, rpf, bn, sub=sub, padded=padded, coff=coff, x=x)
    w = ops.inp('w', torch.randn(K, N, generator=g) / np.sqrt(K), BF if bf else F32T)
    bias = ops.inp('bias', torch.randn(N, generator=g) * 0.1)
    a = abi.PointMlpFwdArgs()
    a.a, a.w, a.bias = src, fptr(w), fptr(bias)
    ref = (rb(act) if bf else act) @ w.double() + bias.double()
    if rowbias:
        rbv = ops.inp('rowbias', torch.randn(B, N, generator=g))
        a.rowbias = fptr(rbv)
        ref = ref + rbv.double().repeat_interleave(rpf, 0)
    o = dict(psum=ops.out('psum', (T, N)), psumsq=ops.out('psumsq', (T, N)))
    a.psum, a.psumsq = fptr(o['psum']), fptr(o['psumsq'])
    if store_y:
        o['y'] = ops.out('y', (M, N), BF if bf else F32T)
        a.y = fptr(o['y'])
    keep = torch.ones(M, dtype=torch.bool, device=DEV)
    if pool:
        for k in ('pmax', 'pmin'):
            o[k] = ops.out(k, (T, N))
        for k in ('pamax', 'pamin'):
            o[k] = ops.out(k, (T, N), torch.int32)
        a.pmax, a.pmin, a.pamax, a.pamin = fptr(o['pmax']), fptr(o['pmin']), iptr(o['pamax']), iptr(o['pamin'])
        if mask:
            m = (torch.rand(M, generator=g) < 0.4).float()
            m[:128] = 0                                                   # one tile with no kept row
            mv = ops.inp('rowmask', m)
            a.rowmask = fptr(mv)
            keep = mv > 0
    a.M, a.K, a.N, a.rows_per_frustum, a.dtype = M, K, N, rpf, abi.BF16 if bf else abi.F32
    assert lib.t3d_pointmlp_fwd(C.byref(a), stream()) == 0
    ops.verify()
    # ---- results
    if store_y:
        assert_clean('y', o['y'], ref)
    rt = ref.reshape(T, 128, N)
    assert_clean('psum', o['psum'], rt.sum(1))
    assert_clean('psumsq', o['psumsq'], (rt * rt).sum(1))
    kt = keep.reshape(T, 128, 1)
    has = kt.any(1).expand(T, N)
    if bf:
        if store_y:
            close_bf16(o['y'], ref, 'y', opmax=float(act.abs().max() * w.double().abs().max()))
            rt = o['y'].double().reshape(T, 128, N)      # statistics and pool candidates of the value as it is stored
        _sums_close_bf16(o['psum'], rt.sum(1), float(rt.abs().sum(1).max()), 'psum')
        _sums_close_bf16(o['psumsq'], (rt * rt).sum(1), float((rt * rt).sum(1).max()), 'psumsq')
    else:
        _close(ref.cpu(), o['y'].cpu(), 2e-5, 2e-5, 'y') if store_y else None
        _close(rt.sum(1).cpu(), o['psum'].cpu(), 1e-4, 2e-3, 'psum')
        _close((rt * rt).sum(1).cpu(), o['psumsq'].cpu(), 1e-4, 2e-3, 'psumsq')
    if pool:
        mx = torch.where(kt, rt, torch.full_like(rt, -np.inf)).max(1).values
        mn = torch.where(kt, rt, torch.full_like(rt, np.inf)).min(1).values
        assert bool(((o['pamax'] >= 0) == has).all()) and bool(((o['pamin'] >= 0) == has).all())
        assert int(has.sum()) > 0
        for got, want, what in ((o['pmax'], mx, 'pmax'), (o['pmin'], mn, 'pmin')):
            assert_clean(what, got[has], want[has])
            if bf:
                assert float((got.double() - want)[has].abs().max()) < 1e-4 * float(rt.abs().max()), what
            else:
                _close(want[has].cpu(), got[has].cpu(), 2e-5, 2e-5, what)
    return o, keep, ref


def _id(v):
    return v if isinstance(v, str) else None


@pytest.mark.parametrize('M,K,N,rpf,kind,kw,why', [
    # !xh && K <= 4 && y && !pmax && !rowbias && N in {64, 128} && coff + 4 <= ldx  ->  k_pointmlp_fwd_tinyk<N> (bf16 y)
    (256, 3, 64, 128, 'raw', dict(coff=0), 'tinyk<64> coff0'), (256, 3, 64, 128, 'raw', dict(coff=4), 'tinyk<64> coff4'),
    (256, 3, 64, 128, 'raw', dict(coff=4, sub=True), 'tinyk<64> sub coff4'), (256, 3, 64, 128, 'raw', dict(coff=0, sub=True), 'tinyk<64> sub coff0'),
    (256, 4, 128, 128, 'raw', dict(coff=0), 'tinyk<128> coff0'), (256, 4, 128, 128, 'raw', dict(coff=4), 'tinyk<128> coff4'),
    (256, 3, 128, 128, 'raw', dict(coff=4, sub=True), 'tinyk<128> sub coff4'),
    # xh && !sub && K in {64, 128}  ->  k_pointmlp_fwd_res<N % 128 ? 64 : 128, K / 64>
    (256, 64, 64, 128, 'bf16', {}, 'fwd_res<64,1>'), (256, 128, 192, 128, 'bf16', {}, 'fwd_res<64,2>'),
    (256, 64, 256, 128, 'bf16', {}, 'fwd_res<128,1>'), (256, 128, 128, 128, 'bf16', {}, 'fwd_res<128,2>'),
    (256, 64, 64, 128, 'bf16', dict(rowbias=True), 'fwd_res<64,1> rowbias'), (256, 128, 192, 128, 'bf16', dict(rowbias=True), 'fwd_res<64,2> rowbias'),
    (256, 64, 256, 128, 'bf16', dict(rowbias=True), 'fwd_res<128,1> rowbias'),
    (256, 128, 128, 128, 'bf16', dict(rowbias=True, pool=True, mask=True, store_y=False), 'fwd_res<128,2> rowbias pool mask(empty tile)'),
    (256, 128, 128, 128, 'bf16', dict(rowbias=True), 'fwd_res<128,2> rowbias'),
    # xh, K not in {64, 128}  ->  k_pointmlp_fwd<64, false, PathBF16, bf16_t>
    (256, 256, 64, 128, 'bf16', {}, 'generic bf16 src K256 N64'), (256, 192, 192, 128, 'bf16', {}, 'generic bf16 src K192 N192'),
    (256, 512, 64, 128, 'bf16', {}, 'generic bf16 src K512 N64'), (256, 256, 192, 128, 'bf16', dict(rowbias=True), 'generic bf16 src K256 N192 rowbias'),
    (256, 192, 64, 128, 'bf16', {}, 'generic bf16 src K192 N64'), (256, 512, 192, 128, 'bf16', {}, 'generic bf16 src K512 N192'),
    # !xh && !sub && K > 4  ->  k_pointmlp_fwd<64, false, PathBF16, float>
    (256, 12, 64, 128, 'f32', {}, 'generic f32 src K12'), (256, 64, 64, 128, 'f32', {}, 'generic f32 src K64'),
    # sub, and not the register kernel (N = 192; pooled)  ->  k_pointmlp_fwd<64, true, PathBF16, float>
    (256, 3, 192, 128, 'raw', dict(coff=4, sub=True), 'generic sub N192'),
    (256, 3, 64, 128, 'raw', dict(coff=0, sub=True, pool=True, mask=True), 'generic sub pooled'),
    (256, 256, 512, 128, 'bf16', dict(pool=True, store_y=False), 'generic pooled nomask'),
    # N % 128 == 0 && tiles_m * N / 128 >= 512 (128 x 4 = 512, the threshold) && K = 256  ->  k_pointmlp_fwd<128, false, PathBF16, bf16_t>
    (16384, 256, 512, 1024, 'bf16', {}, 'generic 128-wide'),
], ids=_id)
def test_forward_bf16(hip_lib, M, K, N, rpf, kind, kw, why):
    run_fwd(hip_lib, M, K, N, rpf, True, kind, **kw)


@pytest.mark.parametrize('M,K,N,rpf,kind,kw,arith,why', [
    # K <= 4 && y && !pmax && !rowbias && N in {64, 128}  ->  k_pointmlp_fwd_tinyk<N, float>, ahead of the arithmetic rule
    (256, 3, 64, 128, 'raw', dict(coff=0), None, 'tinyk<64,float> coff0'), (256, 3, 64, 128, 'raw', dict(coff=4), None, 'tinyk<64,float> coff4'),
    (256, 3, 64, 128, 'raw', dict(coff=4, sub=True), None, 'tinyk<64,float> sub coff4'),
    (256, 4, 128, 128, 'raw', dict(coff=0), None, 'tinyk<128,float> coff0'), (256, 4, 128, 128, 'raw', dict(coff=4), None, 'tinyk<128,float> coff4'),
    (256, 3, 128, 128, 'raw', dict(coff=0, sub=True), None, 'tinyk<128,float> sub coff0'),
    # sub (never x3), N = 192  ->  k_pointmlp_fwd<64, true>
    (256, 3, 192, 128, 'raw', dict(coff=4, sub=True), None, 'generic sub N192'),
    # K % 32 == 0: x3 forward under 'x3', k_pointmlp_fwd<64, false> under fp32_mfma
    (256, 64, 256, 128, 'f32', dict(rowbias=True, pool=True, mask=True), 'x3', 'rowbias pool mask x3'),
    (256, 64, 256, 128, 'f32', dict(rowbias=True, pool=True, mask=True), 'fp32_mfma', 'rowbias pool mask fp32_mfma'),
    # !y && pmax && !sub && N % 128 == 0 && N >= 256 && K == 128  ->  k_pointmlp_fwd_pool<128, 32, 8> (fp32_mfma; x3 goes first under 'x3')
    (256, 128, 256, 128, 'f32', dict(rowbias=True, pool=True, mask=True, store_y=False), 'x3', 'y=NULL pool x3'),
    (256, 128, 256, 128, 'f32', dict(rowbias=True, pool=True, mask=True, store_y=False), 'fp32_mfma', 'fwd_pool<128,32>'),
    # N % 128 == 0 && tiles_m * N / 128 >= 512  ->  k_pointmlp_fwd<128, false>
    (16384, 64, 512, 1024, 'f32', {}, 'fp32_mfma', '128-wide fp32_mfma'),
], ids=_id)
def test_forward_fp32(hip_lib, monkeypatch, M, K, N, rpf, kind, kw, arith, why):
    _arith(monkeypatch, arith)
    run_fwd(hip_lib, M, K, N, rpf, False, kind, **kw)


def test_the_bands_detect_on_the_device(hip_lib):
    """Not vacuous on the GPU either.  The register forward (k_pointmlp_fwd_tinyk<64, float>) launched with `coff` four columns
    too far reads a row's NaN padding (still inside the allocation): assert_clean must name y.  Launched with `y` eight elements
    ahead of the operand, it stores into the front band and leaves the tail unwritten: the checker must name that."""
    M, K, N, rpf = 256, 3, 64, 128
    g = torch.Generator(device='cpu').manual_seed(5)

    def launch(coff_shift, y_shift):
        ops = Ops()
        src, act = make_act(ops, g, M, K, 'raw', rpf, False, coff=0)
        src.coff += coff_shift
        w, bias = ops.inp('w', torch.randn(K, N, generator=g)), ops.inp('bias', torch.randn(N, generator=g))
        y, psum, psumsq = ops.out('y', (M, N)), ops.out('psum', (M // 128, N)), ops.out('psumsq', (M // 128, N))
        a = abi.PointMlpFwdArgs()
        a.a, a.w, a.bias, a.psum, a.psumsq = src, fptr(w), fptr(bias), fptr(psum), fptr(psumsq)
        a.y = C.cast(C.c_void_p(y.data_ptr() + 4 * y_shift), abi.F)
        a.M, a.K, a.N, a.rows_per_frustum = M, K, N, rpf
        assert hip_lib.t3d_pointmlp_fwd(C.byref(a), stream()) == 0
        return ops, y, act @ w.double() + bias.double()

    ops, y, ref = launch(0, 0)
    ops.verify()
    assert_clean('y', y, ref)
    ops, y, ref = launch(4, 0)
    ops.verify()
    with pytest.raises(AssertionError, match='y: .* non-finite'):
        assert_clean('y', y, ref)
    ops, y, ref = launch(0, -8)
    with pytest.raises(AssertionError, match='y: 8 store.s. BEFORE the operand, nearest 1 element'):
        ops.verify()
    with pytest.raises(AssertionError, match='y: 8 element.s. never written'):
        ops.checks['y'].buf[:256] = ops.checks['psum'].buf[:256]          # (put the front band back: the sentinel is one pattern per type)
        ops.checks['y'](written=True)


# ================================================================================================ data gradient
def run_dgrad(lib, M, K, N, rpf, bf, addin, prev, pooled=False, seed=0):
    g = torch.Generator(device='cpu').manual_seed(1000 * seed + M + K + N + 1)
    T, dt = M // 128, BF if bf else F32T
    ops = Ops()
    dsrc, dy = make_dy(ops, g, M, N, bf, rpf, pooled)
    w = ops.inp('w', torch.randn(K, N, generator=g) / np.sqrt(N), dt)
    out = ops.out('out', (M, K), dt)
    d = abi.PointMlpDgradArgs()
    d.dy, d.w, d.out = dsrc, fptr(w), fptr(out)
    ref = dy @ w.double().t()
    if addin:
        add = ops.inp('add_in', torch.randn(M, K, generator=g) * 1e-2, dt)
        d.add_in = fptr(add)
        ref = ref + add.double()
    if prev:
        py = ops.inp('prev_y', torch.randn(M, K, generator=g), dt)
        psc, psh = ops.inp('prev_scale', 0.5 + torch.rand(K, generator=g)), ops.inp('prev_shift', torch.randn(K, generator=g) * 0.3)
        s1, s2 = ops.out('psum_dz', (T, K)), ops.out('psum_dzy', (T, K))
        d.prev_y, d.prev_scale, d.prev_shift, d.psum_dz, d.psum_dzy = fptr(py), fptr(psc), fptr(psh), fptr(s1), fptr(s2)
        ref = torch.where(py.double() * psc.double() + psh.double() > 0, ref, torch.zeros_like(ref))
    d.M, d.K, d.N, d.rows_per_frustum, d.dtype = M, K, N, rpf, abi.BF16 if bf else abi.F32
    assert lib.t3d_pointmlp_dgrad(C.byref(d), stream()) == 0
    ops.verify()
    assert_clean('out', out, ref)
    _check_dx(out, ref, bf, float(dy.abs().max() * w.double().abs().max()), (s1, s2, py) if prev else None)


def _check_dx(out, ref, bf, opmax, stats):
    M, K = out.shape
    T = M // 128
    if bf:
        close_bf16(out, ref, 'dX', opmax=opmax)
        if stats:
            s1, s2, py = stats
            o = out.double().reshape(T, 128, K)
            assert_clean('psum_dz', s1, o.sum(1))
            assert_clean('psum_dzy', s2, o.sum(1))
            assert float((s1.double() - o.sum(1)).abs().max()) < 1e-4 * float(o.abs().sum(1).max() + 1e-9)
            assert float((s2.double() - (o * py.double().reshape(T, 128, K)).sum(1)).abs().max()) < 1e-4 * float(o.abs().sum(1).max() + 1e-9)
    else:
        scale = float(ref.abs().max())
        _close(ref.cpu(), out.cpu(), 1e-4, 2e-5 * scale, 'out')
        if stats:
            s1, s2, py = stats
            r = ref.reshape(T, 128, K)
            assert_clean('psum_dz', s1, r.sum(1))
            assert_clean('psum_dzy', s2, r.sum(1))
            _close(r.sum(1).cpu(), s1.cpu(), 1e-3, 1e-3 * scale, 'psum_dz')
            _close((r * py.double().reshape(T, 128, K)).sum(1).cpu(), s2.cpu(), 1e-3, 2e-3 * scale, 'psum_dzy')


@pytest.mark.parametrize('addin,prev', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('M,K,N,rpf,why', [
    # !(K % 128 == 0 && tiles_m * K / 128 >= 512)  ->  k_pointmlp_dgrad<64, false, PathBF16>
    (256, 64, 64, 128, 'dgrad<64> bf16 K64'), (256, 192, 128, 128, 'dgrad<64> bf16 K192'),
    # K % 128 == 0 && 128 * 4 >= 512  ->  k_pointmlp_dgrad<128, false, PathBF16>
    (16384, 512, 64, 1024, 'dgrad<128> bf16'),
], ids=_id)
def test_dgrad_bf16(hip_lib, M, K, N, rpf, why, addin, prev):
    run_dgrad(hip_lib, M, K, N, rpf, True, addin, prev)


@pytest.mark.parametrize('pooled', [False, True], ids=['dense', 'pooled-sparse'])
def test_dgrad_fp32_mfma_128_wide(hip_lib, fp32_mfma, pooled):
    """K % 128 == 0 && tiles_m * K / 128 >= 512 under fp32_mfma  ->  k_pointmlp_dgrad<128, POOLED>"""
    run_dgrad(hip_lib, 16384, 512, 64, 1024, False, True, True, pooled=pooled)


# ================================================================================================ weight gradient
def _plan(lib, M, K, N):
    rps, tk, tn = C.c_int(0), C.c_int(0), C.c_int(0)
    assert lib.t3d_wgrad_plan(M, K, N, C.byref(rps), C.byref(tk), C.byref(tn)) == 0
    return rps.value, tk.value, tn.value


def _expect_tile(lib, M, K, N, rps, tile, bf_src):
    """Fails when the launcher's tile policy moves: off the plan's split wgrad_tile takes tk = K > 64 ? 128 : 64, tn = N % 128 ? 64 :
    128; on it, the plan's tile; a bf16 source with K % tk != 0 then drops to 64-row k-tiles (its loader does not clamp)."""
    prps, ptk, ptn = _plan(lib, M, K, N)
    if rps is None:
        rps, tk, tn = prps, ptk, ptn
    else:
        assert rps != prps, ('the split must differ from t3d_wgrad_plan\'s', rps, prps)
        tk, tn = (128 if K > 64 else 64), (128 if N % 128 == 0 else 64)
    if bf_src and K % tk:
        tk = 64
    assert (tk, tn) == tile, ('expected tile', (tk, tn), tile)
    return rps


def _check_slabs(slabs, a, dy, rps, bf, what='slabs'):
    S, K, N = slabs.shape
    ref = torch.einsum('smk,smn->skn', a.reshape(S, rps, K), dy.reshape(S, rps, N))
    assert_clean(what, slabs, ref)
    if bf:
        M = S * rps
        flip = 2 * 2.0 ** -7 * float(a.abs().max() * dy.abs().max())      # see close_bf16
        err = float((slabs.double() - ref).abs().max())
        assert err < 2e-5 * float(ref.abs().max()) * max(1.0, np.sqrt(rps / 512)) + flip * max(1.0, rps / 65536.0 * 4), (what, err)
        dw, dw_ref = slabs.double().sum(0), ref.sum(0)
        assert float((dw - dw_ref).abs().max()) < 2e-5 * float(dw_ref.abs().max()) * max(1.0, np.sqrt(M / 512)) + \
            flip * max(1.0, M / 65536.0 * 4), what
    else:
        _close(ref.cpu(), slabs.cpu(), 1e-4, 3e-5 * float(ref.abs().max()), what)


def run_wgrad(lib, M, K, N, rpf, rps, bf, kind, *, bn=True, sub=False, pooled=False, coff=None, seed=0):
    g = torch.Generator(device='cpu').manual_seed(1000 * seed + M + K + N + 2)
    ops = Ops()
    src, act = make_act(ops, g, M, K, kind, rpf, bn, sub=sub, coff=coff)
    dsrc, dy = make_dy(ops, g, M, N, bf, rpf, pooled)
    slabs = ops.out('slabs', (M // rps, K, N))
    a = abi.PointMlpWgradArgs()
    a.a, a.dy, a.slabs = src, dsrc, fptr(slabs)
    a.M, a.K, a.N, a.rows_per_frustum, a.rows_per_split = M, K, N, rpf, rps
    assert lib.t3d_pointmlp_wgrad(C.byref(a), stream()) == 0
    ops.verify()
    _check_slabs(slabs, rb(act) if bf else act, dy, rps, bf)


@pytest.mark.parametrize('M,K,N,kind,sub,rps,tile,why', [
    # off the plan's split: k_pointmlp_wgrad<tk, tn, sub, false, PathBF16, XT>, XT = bf16_t / float
    (512, 64, 64, 'bf16', False, 256, (64, 64), 'wgrad<64,64> bf16 src'), (512, 64, 128, 'bf16', False, 256, (64, 128), 'wgrad<64,128> bf16 src'),
    (512, 128, 64, 'bf16', False, 256, (128, 64), 'wgrad<128,64> bf16 src'), (512, 128, 128, 'bf16', False, 256, (128, 128), 'wgrad<128,128> bf16 src'),
    (512, 64, 64, 'f32', False, 256, (64, 64), 'wgrad<64,64> f32 src'), (512, 64, 128, 'f32', False, 256, (64, 128), 'wgrad<64,128> f32 src'),
    (512, 128, 64, 'f32', False, 256, (128, 64), 'wgrad<128,64> f32 src'), (512, 128, 128, 'f32', False, 256, (128, 128), 'wgrad<128,128> f32 src'),
    # the first layer of every net in a bf16 step: fp32 raw points, K <= 4, bf16 dy (tiny_w is fp32-only)
    (512, 3, 64, 'raw', True, 256, (64, 64), 'wgrad<64,64> raw sub'), (512, 3, 128, 'raw', True, 256, (64, 128), 'wgrad<64,128> raw sub'),
    (512, 4, 64, 'raw', False, 256, (64, 64), 'wgrad<64,64> raw'),
    # the plan's own split and tile
    (512, 64, 64, 'bf16', False, None, (64, 64), 'plan (512,64,64)'), (512, 128, 256, 'bf16', False, None, (64, 64), 'plan (512,128,256)'),
    (1024, 256, 512, 'bf16', False, None, (64, 64), 'plan (1024,256,512)'),
    # K % 128 != 0: a bf16 source takes 64-row k-tiles (see the module docstring); an fp32 source keeps 128 (ActLoaderT<.., float> clamps)
    (512, 192, 128, 'bf16', False, 256, (64, 128), 'K192 bf16 src: tk 128 -> 64'), (512, 320, 64, 'bf16', False, 256, (64, 64), 'K320 bf16 src: tk 128 -> 64'),
    (512, 192, 128, 'f32', False, 256, (128, 128), 'K192 f32 src'),
], ids=_id)
def test_wgrad_bf16(hip_lib, M, K, N, kind, sub, rps, tile, why):
    rps = _expect_tile(hip_lib, M, K, N, rps, tile, kind == 'bf16')
    run_wgrad(hip_lib, M, K, N, 128, rps, True, kind, bn=K > 4, sub=sub, coff=4 if kind == 'raw' else None)


@pytest.mark.parametrize('K,N,sub,bn,coff,why', [
    # fp32 dy, dense, K <= 4, N in {64, 128}, fp32 source  ->  k_pointmlp_wgrad_tinyk<N, sub>
    (3, 64, True, False, 4, 'wgrad_tinyk<64,true>'), (3, 64, True, True, 0, 'wgrad_tinyk<64,true> scale/shift'),
    (3, 128, True, False, 0, 'wgrad_tinyk<128,true>'), (3, 128, True, True, 4, 'wgrad_tinyk<128,true> scale/shift'),
    (4, 64, False, False, 4, 'wgrad_tinyk<64,false> coff4'), (4, 128, False, True, 4, 'wgrad_tinyk<128,false> scale/shift'),
], ids=_id)
def test_wgrad_fp32_tinyk(hip_lib, K, N, sub, bn, coff, why):
    run_wgrad(hip_lib, 512, K, N, 128, 256, False, 'raw', bn=bn, sub=sub, coff=coff)


@pytest.mark.parametrize('M,K,N,tile', [(512, 192, 128, (128, 128)), (512, 320, 64, (128, 64))])
def test_wgrad_fp32_mfma_k_not_a_multiple_of_128(hip_lib, fp32_mfma, M, K, N, tile):
    """K % tk != 0 keeps an fp32 layer off the x3 form (ActLoaderE: no clamp) even under 'x3'; here the fp32-MFMA kernel
    k_pointmlp_wgrad<128, tn, false, false>, whose ActLoader clamps the column to roundup4(K) - 4 and masks: a clean pass."""
    rps = _expect_tile(hip_lib, M, K, N, 256, tile, False)
    run_wgrad(hip_lib, M, K, N, 128, rps, False, 'f32')


# ================================================================================================ fused backward
def run_bwd(lib, M, K, N, rpf, bf, addin, rps_mode, padded, expect_one_pass):
    """t3d_pointmlp_bwd.  padded=False: the layer input IS the producer's raw output (prev_y = a.x, ldx = K, coff = 0: what the
    one-pass forms require, front and back bands only); padded=True: a.x is a padded copy of prev_y, which must take the split form.
    rps_mode: 'bwd' = t3d_bwd_plan's split, 'wgrad' = t3d_wgrad_plan's, or a number."""
    g = torch.Generator(device='cpu').manual_seed(M + K + N + 3)
    T, dt = M // 128, BF if bf else F32T
    rps, one = C.c_int(0), C.c_int(0)
    if rps_mode == 'bwd':
        assert lib.t3d_bwd_plan(M, K, N, abi.BF16 if bf else abi.F32, C.byref(rps), C.byref(one)) == 0
        assert one.value == int(expect_one_pass)
        rps = rps.value
    elif rps_mode == 'wgrad':
        rps = _plan(lib, M, K, N)[0]
    else:
        rps = rps_mode
    ops = Ops()
    x = torch.randn(M, K, generator=g)
    src, act = make_act(ops, g, M, K, 'bf16' if bf else 'f32', rpf, True, padded=padded, x=x)
    py = ops.inp('prev_y', x, dt) if padded else ops.checks['x'].view
    # prev_scale / prev_shift: the producer's batch-norm, the same numbers as the source's scale / shift ([K] floats of their own)
    psc = ops.inp('prev_scale', ops.checks['x.scale'].valid[:K].cpu())
    psh = ops.inp('prev_shift', ops.checks['x.shift'].valid[:K].cpu())
    dsrc, dy = make_dy(ops, g, M, N, bf)
    w = ops.inp('w', torch.randn(K, N, generator=g) / np.sqrt(N), dt)
    out, s1, s2 = ops.out('out', (M, K), dt), ops.out('psum_dz', (T, K)), ops.out('psum_dzy', (T, K))
    slabs = ops.out('slabs', (M // rps, K, N))
    d = abi.PointMlpDgradArgs()
    d.dy, d.w, d.out = dsrc, fptr(w), fptr(out)
    d.prev_y, d.prev_scale, d.prev_shift, d.psum_dz, d.psum_dzy = fptr(py), fptr(psc), fptr(psh), fptr(s1), fptr(s2)
    ref = dy @ w.double().t()
    if addin:
        add = ops.inp('add_in', torch.randn(M, K, generator=g) * 1e-2, dt)
        d.add_in = fptr(add)
        ref = ref + add.double()
    d.M, d.K, d.N, d.rows_per_frustum, d.dtype = M, K, N, rpf, abi.BF16 if bf else abi.F32
    wa = abi.PointMlpWgradArgs()
    wa.a, wa.dy, wa.slabs = src, dsrc, fptr(slabs)
    wa.M, wa.K, wa.N, wa.rows_per_frustum, wa.rows_per_split = M, K, N, rpf, rps
    assert lib.t3d_pointmlp_bwd(C.byref(d), C.byref(wa), stream()) == 0
    ops.verify()
    pyv = ops.checks['x'].valid.double()
    ref = torch.where(pyv * psc.double() + psh.double() > 0, ref, torch.zeros_like(ref))
    assert_clean('out', out, ref)
    _check_dx(out, ref, bf, float(dy.abs().max() * w.double().abs().max()), (s1, s2, pyv))
    _check_slabs(slabs, rb(act) if bf else act, dy, rps, bf)


@pytest.mark.parametrize('M,K,N,rpf,bf,addin,rps_mode,padded,one,arith,why', [
    # N = 512: not a one-pass shape  ->  k_pointmlp_bwd<64, tk, tn, PathBF16>
    (256, 64, 512, 128, True, True, 'wgrad', True, False, None, 'split bf16'),
    # bwd1_shape && rps % 128 == 0 && own_x (prev_y == a.x, coff == 0, ldx == K)  ->  k_pointmlp_bwd1<K, N, BM>
    (512, 64, 64, 256, True, True, 'bwd', False, True, None, 'bwd1<64,64,128>'),
    (512, 256, 128, 256, True, True, 'bwd', False, True, None, 'bwd1<256,128,64>'),
    (512, 64, 64, 256, True, True, 'bwd', True, True, None, 'bwd1 shape, padded layout -> split form'),
    (1024, 64, 128, 256, False, False, 'bwd', False, True, 'fp32_mfma', 'bwd1f<64,128>'),
    (1024, 64, 128, 256, False, False, 'bwd', True, True, 'fp32_mfma', 'bwd1f shape, padded layout -> split form'),
    (1024, 64, 128, 256, False, True, 'bwd', True, True, 'x3', 'x3 fused backward, padded layout'),
    # K % 128 != 0 with a bf16 source off the plan's split: 64-row k-tiles (module docstring)
    (512, 192, 128, 128, True, False, 256, True, False, None, 'K192 bf16 fused'), (512, 320, 64, 128, True, True, 256, True, False, None, 'K320 bf16 fused'),
], ids=_id)
def test_fused_backward(hip_lib, monkeypatch, M, K, N, rpf, bf, addin, rps_mode, padded, one, arith, why):
    _arith(monkeypatch, arith)
    if isinstance(rps_mode, int):
        _expect_tile(hip_lib, M, K, N, rps_mode, (64, 128 if N % 128 == 0 else 64), True)
    run_bwd(hip_lib, M, K, N, rpf, bf, addin, rps_mode, padded, one)


# ================================================================================================ Gram forms
@pytest.mark.parametrize('M,K,rpf,bf,padded,arith,why', [
    # bf16, K in {128, 256}, ldx % 8 == 0  ->  k_gram1; dgram1_ok (K = 256, ldx == K, coff == 0, prev_y == a.x, add_live)  ->  k_dgram1
    (512, 128, 256, True, False, None, 'gram1<128,128> + dgrad_gram<64,bf16>'), (512, 256, 128, True, False, None, 'gram1<256,64> + dgram1<256,64>'),
    (512, 256, 128, True, True, None, 'padded layout: gram1 + split dgrad_gram'),
    (512, 64, 128, True, True, None, 'gram<64,64,bf16> + dgrad_gram<64,bf16>'),
    (512, 128, 256, False, True, 'x3', 'fp32 x3 gram + dgrad_gram'), (512, 128, 256, False, True, 'fp32_mfma', 'fp32_mfma gram + dgrad_gram'),
], ids=_id)
def test_gram_forms(hip_lib, monkeypatch, M, K, rpf, bf, padded, arith, why):
    """t3d_pointmlp_gram (t3d_gram_plan's split) and t3d_pointmlp_dgrad_gram with the sparse rows (add_in gated by add_live: rows
    without the flag hold NaN and must never be read; the flags carry INT32_MIN bands)."""
    _arith(monkeypatch, arith)
    g = torch.Generator(device='cpu').manual_seed(M + K + 5)
    T, dt = M // 128, BF if bf else F32T
    rps, one = C.c_int(0), C.c_int(0)
    assert hip_lib.t3d_gram_plan(M, K, abi.BF16 if bf else abi.F32, C.byref(rps), C.byref(one)) == 0
    assert one.value == int(bf and K in (128, 256))
    rps = rps.value
    ops = Ops()
    x = torch.randn(M, K, generator=g)
    src, act = make_act(ops, g, M, K, 'bf16' if bf else 'f32', rpf, True, padded=padded, x=x)
    slabs = ops.out('slabs', (M // rps, K, K))
    ga = abi.PointMlpGramArgs(src, fptr(slabs), M, K, rpf, rps)
    assert hip_lib.t3d_pointmlp_gram(C.byref(ga), stream()) == 0
    ops.verify()
    a = rb(act) if bf else act
    S = M // rps
    ref = torch.einsum('smk,smn->skn', a.reshape(S, rps, K), a.reshape(S, rps, K))
    assert_clean('gram slabs', slabs, ref)
    if bf:
        assert float((slabs.double().sum(0) - ref.sum(0)).abs().max()) < 2e-5 * float(ref.sum(0).abs().max())
        assert float((slabs.double() - ref).abs().max()) < 2e-5 * float(ref.abs().max())
    else:
        _close(ref.cpu(), slabs.cpu(), 1e-4, 1e-5 * float(ref.abs().max()), 'gram slabs')
    # ---- out = (act(a) . P + rowconst + S[live rows]) masked, with the producer's partials
    P = ops.inp('p', torch.randn(K, K, generator=g) / np.sqrt(K))
    rc = ops.inp('rowconst', torch.randn(K, generator=g) * 0.1)
    live = (torch.rand(M, generator=g) < 0.1)
    Sm = torch.where(live[:, None], torch.randn(M, K, generator=g), torch.full((M, K), NAN))
    Sv, lv = ops.inp('add_in', Sm), ops.inp('add_live', live.to(torch.int32), torch.int32)
    py = ops.inp('prev_y', x, dt) if padded else ops.checks['x'].view
    psc = ops.inp('prev_scale', ops.checks['x.scale'].valid[:K].cpu())
    psh = ops.inp('prev_shift', ops.checks['x.shift'].valid[:K].cpu())
    out, s1, s2 = ops.out('out', (M, K), dt), ops.out('psum_dz', (T, K)), ops.out('psum_dzy', (T, K))
    d = abi.PointMlpDgradGramArgs()
    d.a, d.p, d.rowconst, d.add_in, d.add_live = src, fptr(P), fptr(rc), fptr(Sv), iptr(lv)
    d.prev_y, d.prev_scale, d.prev_shift, d.out, d.psum_dz, d.psum_dzy = fptr(py), fptr(psc), fptr(psh), fptr(out), fptr(s1), fptr(s2)
    d.M, d.K, d.rows_per_frustum, d.dtype = M, K, rpf, abi.BF16 if bf else abi.F32
    assert hip_lib.t3d_pointmlp_dgrad_gram(C.byref(d), stream()) == 0
    ops.verify()
    pyv = ops.checks['x'].valid.double()
    Pd = rb(P) if bf else P.double()
    ref = a @ Pd + rc.double() + torch.nan_to_num(Sv.double(), nan=0.0)
    ref = torch.where(pyv * psc.double() + psh.double() > 0, ref, torch.zeros_like(ref))
    assert_clean('out', out, ref)
    _check_dx(out, ref, bf, float(a.abs().max() * Pd.abs().max()), (s1, s2, pyv))


# ================================================================================================ pool arg indices
@pytest.mark.parametrize('M,K,N,rpf,bf,kind,arith,store_y,why', [
    (512, 64, 256, 256, False, 'f32', 'fp32_mfma', True, 'generic k_pointmlp_fwd<64,false>'),
    (512, 64, 256, 256, False, 'f32', 'x3', True, 'x3'),
    (512, 128, 256, 256, False, 'f32', 'fp32_mfma', False, 'pool kernel k_pointmlp_fwd_pool (y: the generic launch, bit-identical by construction)'),
    (512, 64, 128, 256, True, 'bf16', None, True, 'resident k_pointmlp_fwd_res<128,1>'),
    (512, 256, 64, 256, True, 'bf16', None, True, 'bf16 generic'),
], ids=_id)
def test_pool_arg_indices_with_duplicated_rows(hip_lib, monkeypatch, M, K, N, rpf, bf, kind, arith, store_y, why):
    """Frustums are resampled with replacement: a quarter of each tile's rows are bit-identical copies of other rows of the tile.
    y gathered at pamax / pamin equals pmax / pmin bit for bit, the index is an unmasked row of the tile's own frustum, two runs
    give the same index bytes.  WHICH of the tied rows is reported is not asserted (module docstring)."""
    _arith(monkeypatch, arith)
    T = M // 128
    x = torch.randn(M, K, generator=torch.Generator(device='cpu').manual_seed(77)).reshape(T, 128, K)
    x[:, 96:] = x[:, :32]
    x = x.reshape(M, K)
    runs = [run_fwd(hip_lib, M, K, N, rpf, bf, kind, rowbias=True, pool=True, mask=True, store_y=store_y, x=x) for _ in range(2)]
    o, keep, _ = runs[0]
    y = o['y'] if store_y else run_fwd(hip_lib, M, K, N, rpf, bf, kind, rowbias=True, pool=True, mask=True, store_y=True, x=x)[0]['y']
    assert torch.equal(y.reshape(T, 128, N)[:, 96:], y.reshape(T, 128, N)[:, :32]), 'copied rows give bit-identical outputs'
    tile_frustum = (torch.arange(T, device=DEV) * 128 // rpf)[:, None]
    tied_low = []
    for arg, val, name in ((o['pamax'], o['pmax'], 'pamax'), (o['pamin'], o['pmin'], 'pamin')):
        assert torch.equal(arg.view(torch.uint8), runs[1][0][name].view(torch.uint8)), name + ': two runs, different index bytes'
        has = arg >= 0
        row = (tile_frustum * rpf + arg.long()).clamp(min=0)
        assert bool(((arg < rpf) & (row // 128 == torch.arange(T, device=DEV)[:, None]))[has].all()), name + ': row outside its tile'
        assert bool(keep[row][has].all()), name + ': a masked row'
        got = torch.gather(y, 0, row)
        assert torch.equal(got[has].view(torch.int16 if bf else torch.int32), val.to(y.dtype)[has].view(torch.int16 if bf else torch.int32)), name
        # observation only: how often the reported row is the lowest kept row holding that value
        yt = y.reshape(T, 128, N)
        tie = (yt == val.to(y.dtype)[:, None, :]) & keep.reshape(T, 128, 1)
        first = tie.float().argmax(1) + ((torch.arange(T, device=DEV) * 128) % rpf)[:, None]
        tied_low.append(float((first == arg)[has & (tie.sum(1) > 1)].float().mean()))
    print('duplicated rows, %s: lowest tied row reported for max / min in %.3f / %.3f of the tied columns' % (why, tied_low[0], tied_low[1]))
