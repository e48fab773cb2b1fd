"""Shared cases of the rider tests (tests/test_rider_hosts_gpu.py on libt3d.so, tests/test_rider_hosts_cpu.py on fake_t3d.FakeLib).

csrc/rider_dev.h promises that a small op run as a rider -- alone through t3d_run_riders, or by the first `n_wg` workgroups of a GEMM
launch -- gives the bits of its stand-alone launch.  A case here is a function `case(bufs) -> [(entry point, argument struct)]` that
builds its inputs from a fixed seed and takes every tensor it WRITES from `bufs.out`: the three runs that are compared (stand-alone
launches, the set alone, the set inside a host) each get buffers of their own, pre-filled with a NaN bit pattern and fenced by guard
bands of the same pattern, so equality cannot be a leftover and a store beside an output is seen even where it lands on mapped memory.
The argument structs are filled the way tests/test_kernels_gpu.py and tests/test_kernels_glue_gpu.py fill them (same fields, same value
ranges); the tolerances of the fp64 comparison (ORACLE_TOL) are the expressions of those tests, named there.

HOST_FORMS is the table of rider-hosting kernel forms: one row per `_r` instantiation of csrc/pointmlp.hip with the smallest arguments
that select it (tools/rider_forms_table.py prints it for DESIGN.md)."""
import ctypes as C

import numpy as np
import torch

from transferable3d_amd import abi
from transferable3d_amd.abi import fptr, iptr
from transferable3d_amd.schedule import small_op

REPS = 3                      # repetitions of a set: the barrier words must have reset themselves
PAD = 4096                    # guard elements in front of and behind every written tensor (one row of the widest tensor used here)
SENT = 0x7FC0BEEF             # a quiet NaN with a payload, as int32
ERR_ARG, ERR_SHAPE = -1, -2
RIDER_MAX_WG = 32             # csrc/rider_dev.h
FC_CH, CB = 16, 32            # channels per finalizer workgroup (csrc/bn_dev.h), columns per FC workgroup (csrc/fc_dev.h)


class Env:
    """A library and the device its pointers live on: (libt3d.so, cuda) or (FakeLib(), cpu)."""

    def __init__(self, lib, dev):
        self.lib, self.dev = lib, torch.device(dev)

    def stream(self):
        return None if self.dev.type == 'cpu' else C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def sync(self):
        if self.dev.type != 'cpu':
            torch.cuda.synchronize()


class Bufs:
    """The tensors of one run.  `inp`: read only.  `out`: written by a launch -- sentinel-filled, guard bands on both sides."""

    def __init__(self, dev):
        self.dev, self.outs, self.keep = dev, {}, []

    def inp(self, a):
        x = torch.as_tensor(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(x)
        return x

    def out(self, name, shape, dtype=torch.float32, init=None):
        assert name not in self.outs, name
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        size = torch.empty(0, dtype=dtype).element_size()
        n = (int(np.prod(shape)) * size + 3) // 4                         # 32-bit words
        flat = torch.full((PAD + n + PAD,), SENT, dtype=torch.int32, device=self.dev)
        body = flat[PAD:PAD + n].view(dtype)[:int(np.prod(shape))].reshape(shape)
        assert body.data_ptr() % 16 == 0
        if init is not None:
            body.copy_(torch.as_tensor(np.ascontiguousarray(init)).to(self.dev))
        self.outs[name] = (flat, n, init is not None)
        return body

    def snapshot(self):
        return {k: (f.cpu().numpy().copy(), n, pre) for k, (f, n, pre) in self.outs.items()}


def body(snap, name, dtype=np.float32):
    f, n, _ = snap[name]
    return f[PAD:PAD + n].view(dtype)


def check_guards(snap, what):
    for k, (f, n, pre) in snap.items():
        assert (f[:PAD] == SENT).all(), '%s: %s: the guard band in front was written' % (what, k)
        assert (f[PAD + n:] == SENT).all(), '%s: %s: the guard band behind was written' % (what, k)
        if not pre:
            assert (f[PAD:PAD + n] != SENT).any(), '%s: %s: nothing was written' % (what, k)


def assert_same_bits(a, b, what, names=None):
    """Byte equality of every written tensor (guard bands included) of two runs."""
    for k in (names if names is not None else a.keys()):
        assert a[k][1] == b[k][1]
        same = a[k][0] == b[k][0]
        assert same.all(), '%s: %s differs in %d of %d words (first at %d)' % (what, k, int((~same).sum()), same.size, int(np.argmin(same)) - PAD)


def call_op(env, name, a):
    if name == 't3d_pool_bwd_mid':
        rc = env.lib.t3d_pool_bwd_mid(a.slab_base, a.grad_base, a.table_dev, a.n_tensors, a.max_numel, C.byref(a.sparse), env.stream())
    else:
        rc = getattr(env.lib, name)(C.byref(a), env.stream())
    assert rc == 0, (name, rc)


def default_depends(n):
    return [0] + [1] * (n - 1)


def make_set(env, ops, depends=None, plan_rc=0):
    """abi.RiderSet of `ops` with the given `depends` flags, planned by the library, on zeroed barrier words.  Returns (set, words)."""
    depends = default_depends(len(ops)) if depends is None else depends
    rs = abi.RiderSet()
    for k, (name, arg) in enumerate(ops):
        rs.ops[k] = small_op(name, arg, depends=depends[k])
    rs.n_ops = len(ops)
    rc = env.lib.t3d_riders_plan(C.byref(rs))
    assert rc == plan_rc, ('t3d_riders_plan', rc)
    words = torch.zeros(2 * abi.RIDER_MAX_OPS + 2, dtype=torch.int32, device=env.dev)
    rs.sync = C.cast(C.c_void_p(words.data_ptr()), C.POINTER(C.c_uint32))
    rs._keep = (words, ops)
    return rs, words


def check_sync_words(words, depends, reps, what):
    """Rule of csrc/rider_dev.h: barrier i stands in front of op i >= 1 with `depends`; its arrival count has reset itself, its
    generation has moved once per repetition; no barrier gave up."""
    w = words.cpu().numpy().astype(np.int64)
    assert w[2 * abi.RIDER_MAX_OPS] == 0, '%s: a barrier timed out' % what
    for i in range(abi.RIDER_MAX_OPS):
        assert w[2 * i] == 0, '%s: arrival count of barrier %d is %d' % (what, i, w[2 * i])
        want = reps if (0 < i < len(depends) and depends[i]) else 0
        assert w[2 * i + 1] == want, '%s: generation of barrier %d is %d, expected %d' % (what, i, w[2 * i + 1], want)


def run_apart(env, case, reps=REPS):
    b = Bufs(env.dev)
    ops = case(b)
    for _ in range(reps):
        for name, a in ops:
            call_op(env, name, a)
    env.sync()
    return b.snapshot()


def run_alone(env, case, depends=None, reps=REPS):
    b = Bufs(env.dev)
    ops = case(b)
    rs, words = make_set(env, ops, depends)
    for _ in range(reps):
        rc = env.lib.t3d_run_riders(C.byref(rs), env.stream())
        assert rc == 0, ('t3d_run_riders', rc)
    env.sync()
    return b.snapshot(), rs, words


def check_set_alone(env, case, depends=None, what=''):
    """Rules 1-5 for one set run through t3d_run_riders.  Returns the set (for plan assertions)."""
    n = len(case(Bufs(env.dev)))
    depends = default_depends(n) if depends is None else depends
    ref = run_apart(env, case)
    got, rs, words = run_alone(env, case, depends)
    check_guards(ref, what + ' stand-alone')
    check_guards(got, what + ' set alone')
    assert_same_bits(ref, got, what + ': set alone vs stand-alone launches')
    check_sync_words(words, depends, REPS, what)
    return rs


# ---- hosts ------------------------------------------------------------------------------------------------------------------------------
def call_host(env, fn, args, rs):
    rc = getattr(env.lib, fn + '_r')(*[C.byref(a) for a in args], C.byref(rs) if rs is not None else None, env.stream())
    assert rc == 0, (fn + '_r', rc)


def run_host(env, host, reps=REPS):
    """The host launch with riders == NULL."""
    b = Bufs(env.dev)
    fn, args = host(b)
    for _ in range(reps):
        call_host(env, fn, args, None)
    env.sync()
    return b.snapshot()


def run_hosted(env, host, case, depends=None, reps=REPS):
    b = Bufs(env.dev)
    fn, args = host(b)
    ops = case(b)
    rs, words = make_set(env, ops, depends)
    for _ in range(reps):
        call_host(env, fn, args, rs)
    env.sync()
    return b.snapshot(), rs, words


def check_hosted(env, host, case, what, depends=None, host_ref=None, set_ref=None):
    """The `_r` call with a set against the host with riders == NULL and the set alone (itself against the stand-alone launches):
    host outputs and rider outputs bit for bit, guard bands, barrier words."""
    n = len(case(Bufs(env.dev)))
    depends = default_depends(n) if depends is None else depends
    host_ref = run_host(env, host) if host_ref is None else host_ref
    if set_ref is None:
        apart = run_apart(env, case)
        set_ref, _, words0 = run_alone(env, case, depends)
        assert_same_bits(apart, set_ref, what + ': set alone vs stand-alone launches')
        check_sync_words(words0, depends, REPS, what + ' (alone)')
    got, rs, words = run_hosted(env, host, case, depends)
    check_guards(host_ref, what + ' host alone')
    check_guards(got, what + ' hosted')
    assert_same_bits(host_ref, got, what + ': host outputs, riders == NULL vs hosted', names=host_ref.keys())
    assert_same_bits(set_ref, got, what + ': rider outputs, set alone vs hosted', names=set_ref.keys())
    check_sync_words(words, depends, REPS, what + ' (hosted)')
    return rs


# ---- A. the rider kinds ---------------------------------------------------------------------------------------------------------------------
def bn_fwd_case(N, n_tiles, pool, seed=1, tag=''):
    """t3d_bn_fwd_finalize (test_bn_finalizers_many_tiles' inputs); pool: the fused pool pick, 8 tiles per frustum."""
    r = np.random.RandomState(seed + N + n_tiles)
    T, tpf = n_tiles, 8
    B, M = T // tpf, T * 128
    psum = (r.normal(size=(T, N)) * 30).astype(np.float32)
    psumsq = (np.abs(r.normal(size=(T, N))) * 128 + psum.astype(np.float64) ** 2 / 128).astype(np.float32)
    gamma, beta = r.normal(size=N).astype(np.float32), r.normal(size=N).astype(np.float32)
    mm, mv = r.normal(size=N).astype(np.float32), (0.5 + r.uniform(size=N)).astype(np.float32)
    pmax = r.normal(size=(T, N)).astype(np.float32)
    pmin = (pmax - np.abs(r.normal(size=(T, N)))).astype(np.float32)
    pamax = (r.randint(0, 128, size=(T, N)) + (np.arange(T) % tpf)[:, None] * 128).astype(np.int32)
    pamin = (r.randint(0, 128, size=(T, N)) + (np.arange(T) % tpf)[:, None] * 128).astype(np.int32)
    dead = r.uniform(size=(T, N)) < 0.3
    pamax[dead] = -1
    pamin[dead] = -1

    def case(b):
        f = abi.BnFwdFinalizeArgs()
        f.psum, f.psumsq, f.n_tiles, f.count, f.N = fptr(b.inp(psum)), fptr(b.inp(psumsq)), T, M, N
        f.gamma, f.beta, f.decay = fptr(b.inp(gamma)), fptr(b.inp(beta)), fptr(b.inp(np.array([0.7], np.float32)))
        f.moving_mean, f.moving_var = fptr(b.out(tag + 'mm', N, init=mm)), fptr(b.out(tag + 'mv', N, init=mv))
        f.eps, f.is_training, f.unbiased_ema = 1e-3, 1, 1
        f.scale, f.shift, f.mean, f.invstd = (fptr(b.out(tag + k, N)) for k in ('scale', 'shift', 'mean', 'invstd'))
        if pool:
            f.pool_pmax, f.pool_pmin, f.pool_pamax, f.pool_pamin = fptr(b.inp(pmax)), fptr(b.inp(pmin)), iptr(b.inp(pamax)), iptr(b.inp(pamin))
            f.pool_B, f.pool_tiles_per_frustum, f.ld_pooled = B, tpf, N
            f.pooled, f.argidx, f.ysel = fptr(b.out(tag + 'pooled', (B, N))), iptr(b.out(tag + 'argidx', (B, N), torch.int32)), fptr(b.out(tag + 'ysel', (B, N)))
        return [('t3d_bn_fwd_finalize', f)]
    return case


def bn_bwd_case(N, n_tiles, dense, B=8, seed=2, tag=''):
    """t3d_bn_bwd_finalize in its `coef` form: dense (psum_dz / psum_dzy over n_tiles) or pooled (no psum_dz: dpool_in, pooled, ysel)."""
    r = np.random.RandomState(seed + N + n_tiles)
    T, M = n_tiles, n_tiles * 128
    s1, s2 = r.normal(size=(T, N)).astype(np.float32), r.normal(size=(T, N)).astype(np.float32)
    gamma, scale = r.normal(size=N).astype(np.float32), r.normal(size=N).astype(np.float32)
    mean, invstd = r.normal(size=N).astype(np.float32), (0.5 + r.uniform(size=N)).astype(np.float32)
    dpin, ysel = r.normal(size=(B, N)).astype(np.float32), r.normal(size=(B, N)).astype(np.float32)
    pooled = np.maximum(r.normal(size=(B, N)), 0).astype(np.float32)

    def case(b):
        a = abi.BnBwdFinalizeArgs()
        if dense:
            a.psum_dz, a.psum_dzy, a.n_tiles = fptr(b.inp(s1)), fptr(b.inp(s2)), T
        else:
            a.dpool_in, a.ld_dpool_in, a.pooled, a.ld_pooled = fptr(b.inp(dpin)), N, fptr(b.inp(pooled)), N
            a.ysel, a.dpool, a.B = fptr(b.inp(ysel)), fptr(b.out(tag + 'dpool', (B, N))), B
        a.count, a.N = M, N
        a.gamma, a.mean, a.invstd, a.scale = fptr(b.inp(gamma)), fptr(b.inp(mean)), fptr(b.inp(invstd)), fptr(b.inp(scale))
        a.dgamma, a.dbeta, a.coef = fptr(b.out(tag + 'dgamma', N)), fptr(b.out(tag + 'dbeta', N)), fptr(b.out(tag + 'coef', (3, N)))
        return [('t3d_bn_bwd_finalize', a)]
    return case


def fc_fwd_args(b, x, K, N, B, r, bn, drop, act='relu', tag=''):
    """One FC layer (test_fc_fwd_bwd_dinput's struct) reading the device tensor `x`; returns (struct, out tensor, saved tensors)."""
    w, bias = (r.normal(size=(K, N)) / np.sqrt(K)).astype(np.float32), (r.normal(size=N) * 0.1).astype(np.float32)
    gamma, beta = (0.5 + r.uniform(size=N)).astype(np.float32), (r.normal(size=N) * 0.1).astype(np.float32)
    mm, mv = (r.normal(size=N) * 0.1).astype(np.float32), (0.5 + r.uniform(size=N)).astype(np.float32)
    mask = (r.uniform(size=(B, N)) < 0.7).astype(np.float32)
    a = abi.FcFwdArgs()
    a.in_, a.ld_in, a.K, a.w, a.bias = fptr(x), K, K, fptr(b.inp(w)), fptr(b.inp(bias))
    if bn:
        a.gamma, a.beta = fptr(b.inp(gamma)), fptr(b.inp(beta))
        a.moving_mean, a.moving_var = fptr(b.out(tag + 'mm', N, init=mm)), fptr(b.out(tag + 'mv', N, init=mv))
        a.mean, a.invstd = fptr(b.out(tag + 'mean', N)), fptr(b.out(tag + 'invstd', N))
    a.decay, a.eps, a.is_training, a.unbiased_ema = fptr(b.inp(np.array([0.6], np.float32))), 1e-3, 1, 1
    a.act, a.leaky_alpha = abi.ACT_BY_NAME[act], 0.2
    if drop:
        a.drop_mask, a.keep_prob = fptr(b.inp(mask)), 0.7
    y, out = b.out(tag + 'y', (B, N)), b.out(tag + 'out', (B, N))
    a.y, a.out, a.ld_out, a.B, a.N = fptr(y), fptr(out), N, B, N
    return a, out


def fc_fwd_case(B, K, N, bn, drop, seed=3):
    xs = np.random.RandomState(seed + B + N).normal(size=(B, K)).astype(np.float32)

    def case(b):
        r = np.random.RandomState(seed + 7 * B + N)
        a, _ = fc_fwd_args(b, b.inp(xs), K, N, B, r, bn, drop)
        return [('t3d_fc_fwd', a)]
    return case


def fc_chain_case(B, dims, seed, tag='fc'):
    """The dependent chain of tests/test_riders_gpu.py `_fc_chain` (FC + batch-norm + ReLU, in -> h1 -> h2 ...) on guarded buffers:
    every op reads what the previous one wrote, through another workgroup's stores."""
    def case(b):
        r = np.random.RandomState(seed)
        cur = b.inp(r.randn(B, dims[0]).astype(np.float32))
        ops = []
        for k, (K, N) in enumerate(zip(dims[:-1], dims[1:])):
            a, cur = fc_fwd_args(b, cur, K, N, B, r, True, False, tag='%s%d.' % (tag, k))
            ops.append(('t3d_fc_fwd', a))
        return ops
    return case


FC_CHAIN = dict(B=32, dims=(256, 512, 512, 256, 64), seed=7)      # the 4-op set of test_riders_gpu.py


def _fc_saved(r, B, N, bn, drop, act='relu'):
    """Saved activations of a forward layer, consistent with one another (y, mean, invstd, out)."""
    y = r.normal(size=(B, N)).astype(np.float32)
    gamma, beta = (0.5 + r.uniform(size=N)).astype(np.float32), (r.normal(size=N) * 0.1).astype(np.float32)
    mean = y.mean(0).astype(np.float32)
    invstd = (1.0 / np.sqrt(y.var(0) + 1e-3)).astype(np.float32)
    mask = (r.uniform(size=(B, N)) < 0.7).astype(np.float32)
    z = (y - mean) * invstd * gamma + beta if bn else y
    out = np.maximum(z, 0) if act == 'relu' else z
    if drop:
        out = out * mask / 0.7
    return y, gamma, beta, mean, invstd, mask, out.astype(np.float32)


def fc_bwd_args(b, r, B, K, N, bn, drop, dout=None, nxt=None, x=None, act='relu', tag=''):
    """t3d_fc_bwd (test_fc_fwd_bwd_dinput's struct).  dout: device tensor [B, N]; nxt = (dy_next [B, Nn], w_next [N, Nn], Nn)."""
    y, gamma, beta, mean, invstd, mask, out = _fc_saved(r, B, N, bn, drop, act)
    xs = r.normal(size=(B, K)).astype(np.float32)
    a = abi.FcBwdArgs()
    if nxt is not None:
        a.dy_next, a.w_next, a.N_next = fptr(nxt[0]), fptr(nxt[1]), nxt[2]
    else:
        a.dout, a.ld_dout = fptr(dout), N
    a.in_, a.ld_in, a.K = fptr(b.inp(xs) if x is None else x), K, K
    a.y, a.out, a.ld_out = fptr(b.inp(y)), fptr(b.inp(out)), N
    if bn:
        a.gamma, a.beta, a.mean, a.invstd = fptr(b.inp(gamma)), fptr(b.inp(beta)), fptr(b.inp(mean)), fptr(b.inp(invstd))
    a.bn_training, a.act, a.leaky_alpha = 1, abi.ACT_BY_NAME[act], 0.2
    if drop:
        a.drop_mask, a.keep_prob = fptr(b.inp(mask)), 0.7
    dy = b.out(tag + 'dy', (B, N))
    a.dy, a.dw, a.dbias = fptr(dy), fptr(b.out(tag + 'dw', (K, N))), fptr(b.out(tag + 'db', N))
    if bn:
        a.dgamma, a.dbeta = fptr(b.out(tag + 'dgamma', N)), fptr(b.out(tag + 'dbeta', N))
    a.B, a.N = B, N
    return a, dy


def fc_bwd_case(B, K, N, bn, drop, seed=4):
    def case(b):
        r = np.random.RandomState(seed + 7 * B + N)
        a, _ = fc_bwd_args(b, r, B, K, N, bn, drop, dout=b.inp(r.normal(size=(B, N)).astype(np.float32)))
        return [('t3d_fc_bwd', a)]
    return case


def fc_dinput_args(b, r, dy, B, N, K, bn, tag=''):
    """t3d_fc_dinput: din = alpha * dy . w^T + add_in; bn: with the fused pooled batch-norm backward
    (test_fc_dinput_with_fused_pooled_bn_bwd's struct)."""
    w = (r.normal(size=(K, N)) / np.sqrt(N)).astype(np.float32)
    a = abi.FcDinputArgs()
    din = b.out(tag + 'din', (B, K))
    a.dy, a.N, a.w, a.din, a.ld_din, a.B, a.K = fptr(dy), N, fptr(b.inp(w)), fptr(din), K, B, K
    if bn:
        a.alpha = 1.0
        a.bn_pooled, a.bn_ld_pooled = fptr(b.inp(np.maximum(r.normal(size=(B, K)), 0).astype(np.float32))), K
        a.bn_ysel, a.bn_dpool, a.bn_count = fptr(b.inp(r.normal(size=(B, K)).astype(np.float32))), fptr(b.out(tag + 'dpool', (B, K))), B * 1024
        a.bn_gamma, a.bn_mean = fptr(b.inp((0.5 + r.uniform(size=K)).astype(np.float32))), fptr(b.inp(r.normal(size=K).astype(np.float32)))
        a.bn_invstd, a.bn_scale = fptr(b.inp((0.5 + r.uniform(size=K)).astype(np.float32))), fptr(b.inp(r.normal(size=K).astype(np.float32)))
        a.bn_dgamma, a.bn_dbeta, a.bn_coef = fptr(b.out(tag + 'bn_dg', K)), fptr(b.out(tag + 'bn_db', K)), fptr(b.out(tag + 'bn_coef', (3, K)))
    else:
        a.add_in, a.ld_add, a.alpha = fptr(b.inp(np.full((B, K), 0.5, np.float32))), K, -1.0
    return a, din


def fc_dinput_case(B, N, K, bn, seed=5):
    def case(b):
        r = np.random.RandomState(seed + 7 * B + K)
        a, _ = fc_dinput_args(b, r, b.inp(r.normal(size=(B, N)).astype(np.float32)), B, N, K, bn)
        return [('t3d_fc_dinput', a)]
    return case


def dy_colsum_case(B, N, tpf=2, seed=6):
    r = np.random.RandomState(seed + B + N)
    T = B * tpf
    s1, psum, coef = r.normal(size=(T, N)).astype(np.float32), (r.normal(size=(T, N)) * 128).astype(np.float32), r.normal(size=(3, N)).astype(np.float32)

    def case(b):
        a = abi.DyColsumArgs(fptr(b.inp(s1)), fptr(b.inp(psum)), fptr(b.inp(coef)), B, N, tpf, tpf * 128, -1.0, fptr(b.out('colsum', (B, N))))
        return [('t3d_dy_colsum', a)]
    return case


MID_SHAPES = [(512, 128, 1024, 256), (256, 256, 512, 128)]      # test_pool_bwd_mid_equals_reduce_slabs_then_sparse_rows
MID_SLABS = [(70, 640), (9, 36992), (3, 67)]                     # (n_slabs, numel) of that test


def pool_bwd_mid_case(M, K, N, rpf, seed=None):
    """The wide rider: t3d_pool_bwd_mid with the slab table and the `_pool_case` inputs of the stand-alone test."""
    r = np.random.RandomState(M + N if seed is None else seed)
    slab = np.concatenate([r.normal(size=ns * ne) for ns, ne in MID_SLABS]).astype(np.float32)
    table = (abi.SlabDesc * 3)()
    so, go = 0, 8
    for i, (ns, ne) in enumerate(MID_SLABS):
        table[i] = abi.SlabDesc(so, go, ne, ns)
        so += ns * ne
        go += ne + 4
    B = M // rpf
    hot = r.randint(0, rpf, size=(B, 24))
    argidx = np.take_along_axis(hot, r.randint(0, 24, size=(B, N)), 1).astype(np.int32)
    argidx[r.uniform(size=(B, N)) < 0.1] = -1
    argidx[0, :N // 2] = 5
    dpool, wc = r.normal(size=(B, N)).astype(np.float32), (r.normal(size=(N, K)) / np.sqrt(K)).astype(np.float32)
    live = np.zeros(go, bool)
    for i in range(3):
        live[table[i].grad_off:table[i].grad_off + table[i].numel] = True

    def case(b):
        a = abi.PoolBwdMidArgs()
        grad = b.out('mid.grad', go, init=np.full(go, -3.5, np.float32))      # (the gaps between the tensors stay -3.5)
        tab_dev = b.inp(np.frombuffer(bytes(table), dtype=np.uint8).copy())
        a.slab_base, a.grad_base = fptr(b.inp(slab)), fptr(grad)
        a.table_dev = table if b.dev.type == 'cpu' else C.cast(C.c_void_p(tab_dev.data_ptr()), C.POINTER(abi.SlabDesc))
        a.n_tensors, a.max_numel = 3, max(ne for _, ne in MID_SLABS)
        a.sparse = abi.PoolSparseRowsArgs(iptr(b.inp(argidx)), fptr(b.inp(dpool)), fptr(b.inp(wc)), B, N, K, rpf, fptr(b.out('mid.s', (M, K))), None)
        a._keep = table
        return [('t3d_pool_bwd_mid', a)]
    case.gaps = ~live
    return case


def mid_blocks(M, K):
    """Workgroups of the wide rider (csrc/rider_dev.h mid_gx, mid_sparse_blocks): slab-reduction blocks per tensor, then sparse-row tiles."""
    mx = max(ne for _, ne in MID_SLABS)
    gx = min(256, max(1, (mx // 4 + 31) // 32))
    return gx * len(MID_SLABS) + (M // 128) * (K // 128)


def sparse_rows_lds(N):
    return 128 * 128 * 4 + (4 * N + 128) * 4      # csrc/poolbwd_dev.h


# cases of part A: (id, case factory, arguments)
KIND_CASES = (
    [('bn_fwd-N%d-T%d-%s' % (N, T, 'pool' if p else 'plain'), bn_fwd_case, (N, T, p))
     for N, T, p in [(16, 8, False), (16, 512, True), (1024, 8, True), (1024, 512, False)]] +
    [('bn_bwd-N%d-T%d-%s' % (N, T, 'dense' if d else 'pooled'), bn_bwd_case, (N, T, d))
     for N, T, d in [(16, 8, True), (16, 512, False), (1024, 8, False), (1024, 512, True)]] +
    [('fc_fwd-B%d-N%d-bn%d-drop%d' % (B, N, bn, dr), fc_fwd_case, (B, 64, N, bn, dr))
     for B, N, bn, dr in [(1, 32, 0, 0), (32, 32, 1, 1), (1, 96, 1, 0), (32, 96, 0, 1), (1, 2048, 0, 1), (32, 2048, 1, 0)]] +
    [('fc_bwd-B%d-N%d-bn%d-drop%d' % (B, N, bn, dr), fc_bwd_case, (B, 64, N, bn, dr))
     for B, N, bn, dr in [(1, 32, 1, 0), (32, 32, 0, 1), (1, 96, 0, 0), (32, 96, 1, 1), (1, 2048, 1, 1), (32, 2048, 0, 0)]] +
    [('fc_dinput-B%d-K%d-bn%d' % (B, K, bn), fc_dinput_case, (B, 64, K, bn))
     for B, K, bn in [(1, 32, 0), (32, 32, 1), (1, 96, 1), (32, 96, 0), (1, 2048, 0), (32, 2048, 1)]] +
    [('dy_colsum-B%d-N%d' % (B, N), dy_colsum_case, (B, N)) for B, N in [(2, 128), (32, 512)]])

# Rule 6: |gpu - fp64 spec| <= atol + rtol * |spec| per written tensor, the expressions of tests/test_kernels_gpu.py:
# test_fc_fwd_bwd_dinput (fc_fwd 2e-4 / 2e-4; fc_bwd 5e-4 / 2e-4 max|ref|; fc_dinput 2e-4 / 2e-4 max|din|), test_bn_finalizers_pool_colsum
# (finalizers 1e-5 / 1e-6; colsum 1e-5 / 1e-4), test_fc_dinput_with_fused_pooled_bn_bwd (din, dpool 1e-5 / 1e-5; dgamma, dbeta 1e-4 / 1e-4;
# coef 1e-4 / 1e-6).  (rtol, atol, atol is relative to max|ref|)
ORACLE_TOL = {
    'bn_fwd': lambda k: (1e-5, 1e-6, False), 'bn_bwd': lambda k: (1e-5, 1e-6, False), 'dy_colsum': lambda k: (1e-5, 1e-4, False),
    'fc_fwd': lambda k: (2e-4, 2e-4, False), 'fc_bwd': lambda k: (5e-4, 2e-4, True),
    'fc_dinput': lambda k: {'din': (2e-4, 2e-4, True), 'dpool': (1e-5, 1e-5, False), 'bn_dg': (1e-4, 1e-4, False), 'bn_db': (1e-4, 1e-4, False),
                            'bn_coef': (1e-4, 1e-6, False)}[k],
}
ORACLE_TOL_FUSED_DIN = (1e-5, 1e-5, False)      # din of the fused form (test_fc_dinput_with_fused_pooled_bn_bwd)


ORACLE_TOL['pool_bwd_mid'] = lambda k: {'grad': (1e-5, 1e-5, False), 's': (1e-5, 1e-5, True)}[k]      # test_pool_bwd_mid_equals_reduce_slabs_then_sparse_rows
ORACLE_KIND = {'t3d_bn_fwd_finalize': 'bn_fwd', 't3d_bn_bwd_finalize': 'bn_bwd', 't3d_fc_fwd': 'fc_fwd', 't3d_fc_bwd': 'fc_bwd',
               't3d_fc_dinput': 'fc_dinput', 't3d_dy_colsum': 'dy_colsum', 't3d_pool_bwd_mid': 'pool_bwd_mid'}


def compare_with_spec(cur, spec, k, kind, fused_din, label, verbose=True, stats=None):
    """One written tensor `k` of a device snapshot against the specification's, with ORACLE_TOL of the op kind that wrote it.  Words the
    specification left at the sentinel (the padding columns of a strided output) must still hold it on the device.  stats: per
    (kind, output) the largest error, the bound at that element, the largest error / bound and the case it came from."""
    key = k.split('.')[-1]
    if key == 'argidx':
        assert (body(cur, k, np.int32) == body(spec, k, np.int32)).mean() > 0.999, (label, k)      # ties between equal maxima
        return
    pad = body(spec, k, np.int32) == SENT
    assert (body(cur, k, np.int32)[pad] == SENT).all(), '%s %s: a padding element was written' % (label, k)
    assert not pad.all(), (label, k)
    got, ref = body(cur, k)[~pad].astype(np.float64), body(spec, k)[~pad].astype(np.float64)
    rtol, atol, rel = ORACLE_TOL[kind](key)
    if kind == 'fc_dinput' and key == 'din' and fused_din:
        rtol, atol, rel = ORACLE_TOL_FUSED_DIN
    if rel:
        atol *= max(float(np.abs(ref).max()), 1e-6)
    err, tol = np.abs(got - ref), atol + rtol * np.abs(ref)
    if verbose:
        print('%s %s: max err %.3g, max |ref| %.3g, worst err / tol %.3g' %
              (label, k, float(err.max()), float(np.abs(ref).max()), float((err / tol).max())))
    if stats is not None:
        j = int(np.argmax(err))
        s = stats.setdefault((kind, key), [0.0, 0.0, -1.0, ''])
        if float(err[j]) >= s[0]:
            s[0], s[1] = float(err[j]), float(tol[j])
        if float((err / tol).max()) > s[2]:
            s[2], s[3] = float((err / tol).max()), label
    assert np.isfinite(ref).all() and (err <= tol).all(), (label, k, float(err.max()), float(np.abs(ref).max()), int((err > tol).sum()))


def check_against_oracle(env_gpu, env_cpu, case, what, verbose=True, stats=None):
    """Every op of a case as ONE stand-alone launch on the device against the fp64 specification ON IDENTICAL INPUTS: the ops run in
    order, and before op i + 1 the specification's buffers take the device's results of op i, so each comparison is of one kernel
    (the tolerance of its own test), not of an error accumulated along a chain."""
    bg, bc = Bufs(env_gpu.dev), Bufs(env_cpu.dev)
    og, oc = case(bg), case(bc)
    prev = bg.snapshot()
    for i, ((name, ag), (_, ac)) in enumerate(zip(og, oc)):
        call_op(env_gpu, name, ag)
        env_gpu.sync()
        call_op(env_cpu, name, ac)
        cur, spec = bg.snapshot(), bc.snapshot()
        written = [k for k in cur if not (cur[k][0] == prev[k][0]).all()]
        assert written, (what, i, name)
        kind = ORACLE_KIND[name]
        for k in written:
            compare_with_spec(cur, spec, k, kind, kind == 'fc_dinput' and bool(ag.bn_pooled), '%s op %d %s' % (what, i, name), verbose, stats)
            bc.outs[k][0].copy_(torch.from_numpy(cur[k][0]))      # the next op reads the device's values on both sides
        prev = cur


# ---- B. sets ----------------------------------------------------------------------------------------------------------------------------
def fc_head_bwd_case(n_ops, B=32, seed=11):
    """Backward of a three-layer FC head, last layer first: fc_bwd (layer 3, from dout) -> fc_bwd (layer 2, from layer 3's dy through
    w3) -> bn_bwd_finalize ... every op reads what its predecessor wrote.  Widths 67 / 256 / 512 / 96 / 2048: 3, 8, 16, 3 and 64
    blocks, so some workgroups have no block of an op and some ops take the stride loop twice.  n_ops: length of the set."""
    def case(b):
        r = np.random.RandomState(seed)
        ops, owners = [], ['l3', 'l2', 'l1', 'd1', 'd2', 'f', 'd3', 'f4', 'f5', 'd4']      # tag of the tensors op i writes
        N3, N2, N1, K1 = 67, 256, 512, 96
        dout = b.inp(r.normal(size=(B, N3)).astype(np.float32))
        w3 = b.inp((r.normal(size=(N2, N3)) / np.sqrt(N2)).astype(np.float32))
        w2 = b.inp((r.normal(size=(N1, N2)) / np.sqrt(N1)).astype(np.float32))
        a3, dy3 = fc_bwd_args(b, r, B, N2, N3, False, False, dout=dout, act=None, tag='l3.')            # 3 blocks
        ops.append(('t3d_fc_bwd', a3))
        a2, dy2 = fc_bwd_args(b, r, B, N1, N2, True, True, nxt=(dy3, w3, N3), tag='l2.')                # 8 blocks, reads dy3
        ops.append(('t3d_fc_bwd', a2))
        a1, dy1 = fc_bwd_args(b, r, B, K1, N1, True, False, nxt=(dy2, w2, N2), tag='l1.')               # 16 blocks, reads dy2
        ops.append(('t3d_fc_bwd', a1))
        d1, din1 = fc_dinput_args(b, r, dy1, B, N1, K1, False, tag='d1.')                                # 3 blocks, reads dy1
        ops.append(('t3d_fc_dinput', d1))
        d2, din2 = fc_dinput_args(b, r, din1, B, K1, 2048, True, tag='d2.')                              # 64 blocks, reads din1; fused bn
        ops.append(('t3d_fc_dinput', d2))
        # pooled batch-norm backward finalizer on the 2048-wide gradient (128 blocks), then layers that read ITS dpool
        f = abi.BnBwdFinalizeArgs()
        N = 2048
        f.dpool_in, f.ld_dpool_in = fptr(din2), N
        f.pooled, f.ld_pooled = fptr(b.inp(np.maximum(r.normal(size=(B, N)), 0).astype(np.float32))), N
        dpool = b.out('f.dpool', (B, N))
        f.ysel, f.dpool, f.B, f.count, f.N = fptr(b.inp(r.normal(size=(B, N)).astype(np.float32))), fptr(dpool), B, B * 1024, N
        f.gamma, f.mean = fptr(b.inp(r.normal(size=N).astype(np.float32))), fptr(b.inp(r.normal(size=N).astype(np.float32)))
        f.invstd, f.scale = fptr(b.inp((0.5 + r.uniform(size=N)).astype(np.float32))), fptr(b.inp(r.normal(size=N).astype(np.float32)))
        f.dgamma, f.dbeta, f.coef = fptr(b.out('f.dgamma', N)), fptr(b.out('f.dbeta', N)), fptr(b.out('f.coef', (3, N)))
        ops.append(('t3d_bn_bwd_finalize', f))
        d3, din3 = fc_dinput_args(b, r, dpool, B, N, 32, False, tag='d3.')                               # 1 block, reads dpool
        ops.append(('t3d_fc_dinput', d3))
        a4, out4 = fc_fwd_args(b, din3, 32, 96, B, r, True, False, tag='f4.')                            # 3 blocks, reads din3
        ops.append(('t3d_fc_fwd', a4))
        a5, out5 = fc_fwd_args(b, out4, 96, 2048, B, r, True, True, tag='f5.')                           # 64 blocks, reads out4
        ops.append(('t3d_fc_fwd', a5))
        d4, _ = fc_dinput_args(b, r, out5, B, 2048, 96, False, tag='d4.')                                # 3 blocks, reads out5
        ops.append(('t3d_fc_dinput', d4))
        assert len(ops) == abi.RIDER_MAX_OPS
        for k in [k for k in b.outs if k.split('.')[0] not in owners[:n_ops]]:      # a shorter set writes the first ops' tensors only
            del b.outs[k]
        return ops[:n_ops]
    return case


def independent_case(pattern, seed=13):
    """len(pattern) ops with disjoint outputs.  Where pattern[i] == 1, op i is an FC layer reading op i-1's output (it needs the barrier);
    where 0 (i > 0) it reads a tensor of its own: `depends` = pattern is then a correct hand-built set."""
    def case(b):
        r = np.random.RandomState(seed)
        B, ops, prev, widths = 32, [], None, (96, 512, 32, 256)
        for i, dep in enumerate(pattern):
            K, N = (widths[i - 1] if dep else 64), widths[i % 4]
            x = prev if dep else b.inp(r.normal(size=(B, K)).astype(np.float32))
            a, prev = fc_fwd_args(b, x, K, N, B, r, True, i % 2 == 1, tag='op%d.' % i)
            ops.append(('t3d_fc_fwd', a))
        return ops
    return case


# ---- C. the rider-hosting forms -----------------------------------------------------------------------------------------------------------
# Column-tile rules of csrc/pointmlp.hip, restated once:
def fwd_wide(M, N):
    """select_fwd / t3d_x3_fwd, csrc/pointmlp.hip `wide_tiles(tiles_m, N)`: `cols % 128 == 0 && (long)tiles_m * (cols / 128) >= 512`"""
    return N % 128 == 0 and (M // 128) * (N // 128) >= 512


def dgrad_wide(M, K):
    """csrc/pointmlp.hip `dgrad_wide` = `wide_tiles(a->M / 128, a->K)` (`dgrad_gram_wide` is the same rule)"""
    return K % 128 == 0 and (M // 128) * (K // 128) >= 512


dgrad_gram_wide = dgrad_wide


def wgrad_tile(lib, M, K, N, rps=None):
    """(rows_per_split, tk, tn) the launchers take (csrc/pointmlp.hip `wgrad_tile`): t3d_wgrad_plan's tile when rows_per_split is the
    plan's, else the documented fallback tk = K > 64 ? 128 : 64, tn = N % 128 == 0 ? 128 : 64."""
    p, tk, tn = C.c_int(0), C.c_int(0), C.c_int(0)
    assert lib.t3d_wgrad_plan(M, K, N, C.byref(p), C.byref(tk), C.byref(tn)) == 0
    if rps is None or rps == p.value:
        return p.value, tk.value, tn.value
    return rps, (128 if K > 64 else 64), (128 if N % 128 == 0 else 64)


F32, X3 = abi.ARITH_FP32_MFMA, abi.ARITH_BF16X3
GEMM_FWD, GEMM_BWD, GEMM_DGRAD, GEMM_WGRAD, GEMM_GRAM, GEMM_DGRAD_GRAM = range(6)      # t3d.h T3D_GEMM_*


def x3_planes(env, w):
    """(forward planes, data-gradient planes, stride) of one [K, N] matrix through t3d_split_x3_frag (test_kernels_gpu._x3_frag_planes)."""
    K, N = w.shape
    stride = (K * N + 7) // 8 * 8
    pf = torch.zeros(3 * stride, dtype=torch.bfloat16, device=w.device)
    pd = torch.zeros(3 * stride, dtype=torch.bfloat16, device=w.device)
    raw, nblk = abi.x3_frag_table([(0, K, N)])
    tab = torch.from_numpy(raw).to(w.device)
    rc = env.lib.t3d_split_x3_frag(fptr(w), C.c_void_p(pf.data_ptr()), C.c_void_p(pd.data_ptr()), stride, C.c_void_p(tab.data_ptr()), 1, nblk, env.stream())
    assert rc == 0, rc
    env.sync()
    return pf, pd, stride


def fwd_host(env, M, K, N, rpf, arith, sub=False, pre=False, dtype=abi.F32, nostore_pool=False):
    """t3d_pointmlp_fwd (test_pointmlp_fwd's struct: 'bn' input transform, or 'sub' on raw points)."""
    r = np.random.RandomState(M + K + N)
    ldx, T, B = (4 if K <= 4 else K), M // 128, M // rpf
    x = r.normal(size=(M, ldx)).astype(np.float32)
    w = (r.normal(size=(K, N)) / np.sqrt(K)).astype(np.float32)
    bias, sc, sh = (r.normal(size=N) * 0.1).astype(np.float32), (0.5 + r.uniform(size=K)).astype(np.float32), (r.normal(size=K) * 0.2).astype(np.float32)
    sc[::3] *= -1
    subv = r.normal(size=(B, 3)).astype(np.float32)

    def host(b):
        a = abi.PointMlpFwdArgs()
        xt, wt = b.inp(x), b.inp(w)
        if dtype == abi.BF16:
            xt = xt.to(torch.bfloat16) if K > 4 else xt
            b.keep.append(xt)
        bn = not sub and K > 4
        a.a = abi.ActSrc(C.cast(C.c_void_p(xt.data_ptr()), abi.F), ldx, 0, fptr(b.inp(sc) if bn else None), fptr(b.inp(sh) if bn else None), int(bn),
                         fptr(b.inp(subv) if sub else None), 3, abi.BF16 if xt.dtype == torch.bfloat16 else abi.F32)
        a.w, a.bias = fptr(wt), fptr(b.inp(bias))
        ydt = torch.bfloat16 if dtype == abi.BF16 else torch.float32
        if nostore_pool:
            a.pmax, a.pmin = fptr(b.out('h.pmax', (T, N))), fptr(b.out('h.pmin', (T, N)))
            a.pamax, a.pamin = iptr(b.out('h.pamax', (T, N), torch.int32)), iptr(b.out('h.pamin', (T, N), torch.int32))
        else:
            a.y = C.cast(C.c_void_p(b.out('h.y', (M, N), ydt).data_ptr()), abi.F)
        a.psum, a.psumsq = fptr(b.out('h.psum', (T, N))), fptr(b.out('h.psumsq', (T, N)))
        a.M, a.K, a.N, a.rows_per_frustum, a.dtype, a.arith = M, K, N, rpf, dtype, arith
        if pre:
            pf, pd, stride = x3_planes(env, wt)
            a.w_x3, a.w_x3_stride = pf.data_ptr(), stride
            b.keep += [pf, pd]
        return 't3d_pointmlp_fwd', (a,)
    host.query = lambda lib, args: lib.t3d_pointmlp_fwd_hosts_riders(C.byref(args[0]))
    return host


def _dense_bwd_inputs(M, K, N):
    r = np.random.RandomState(M + K + N)
    return dict(x=r.normal(size=(M, 4 if K <= 4 else K)).astype(np.float32), sc=(0.5 + r.uniform(size=K)).astype(np.float32),
                sh=(r.normal(size=K) * 0.3).astype(np.float32), w=(r.normal(size=(K, N)) / np.sqrt(N)).astype(np.float32),
                dz=(r.normal(size=(M, N)) * 1e-2).astype(np.float32), y=r.normal(size=(M, N)).astype(np.float32),
                coef=r.normal(size=(3, N)).astype(np.float32), sub=r.normal(size=(M // 128, 3)).astype(np.float32))


def _typed(b, t, dtype):
    """(pointer, tensor) of `t` in the launch's element type (bf16: a rounded copy, kept alive by `b`)"""
    if dtype == abi.BF16:
        t = t.to(torch.bfloat16)
        b.keep.append(t)
    return C.cast(C.c_void_p(t.data_ptr()), abi.F)


def _typed_out(b, name, shape, dtype):
    return C.cast(C.c_void_p(b.out(name, shape, torch.bfloat16 if dtype == abi.BF16 else torch.float32).data_ptr()), abi.F)


def wgrad_host(env, M, K, N, rpf, arith, sub=False, rps=None, dtype=abi.F32):
    """t3d_pointmlp_wgrad (test_pointmlp_wgrad's struct, dense dy)."""
    d = _dense_bwd_inputs(M, K, N)
    rps_, tk, tn = wgrad_tile(env.lib, M, K, N, rps)

    def host(b):
        t = {k: b.inp(v) for k, v in d.items()}
        a = abi.PointMlpWgradArgs()
        bn = not sub and K > 4
        a.a = abi.ActSrc(_typed(b, t['x'], dtype), 4 if K <= 4 else K, 0, fptr(t['sc'] if bn else None), fptr(t['sh'] if bn else None), int(bn),
                         fptr(t['sub'] if sub else None), 3, dtype)
        a.dy = abi.DySrc(_typed(b, t['dz'], dtype), _typed(b, t['y'], dtype), fptr(t['coef']), iptr(None), fptr(None), dtype)
        a.slabs = fptr(b.out('h.slabs', (M // rps_, K, N)))
        a.M, a.K, a.N, a.rows_per_frustum, a.rows_per_split, a.arith = M, K, N, rpf if not sub else 128, rps_, arith
        return 't3d_pointmlp_wgrad', (a,)
    host.query = lambda lib, args: lib.t3d_pointmlp_wgrad_hosts_riders(C.byref(args[0]))
    host.tile = (tk, tn)
    return host


def bwd_host(env, M, K, N, rpf, arith, rps=None, pre=False, dtype=abi.F32):
    """t3d_pointmlp_bwd (test_fused_bwd_equals_separate_dgrad_and_wgrad's structs, 'mask' mode: ReLU mask and statistics)."""
    d = _dense_bwd_inputs(M, K, N)
    rps_, tk, tn = wgrad_tile(env.lib, M, K, N, rps)

    def host(b):
        t = {k: b.inp(v) for k, v in d.items() if k != 'sub'}
        T = M // 128
        xp = _typed(b, t['x'], dtype)
        act = abi.ActSrc(xp, K, 0, fptr(t['sc']), fptr(t['sh']), 1, fptr(None), 0, dtype)
        dy = abi.DySrc(_typed(b, t['dz'], dtype), _typed(b, t['y'], dtype), fptr(t['coef']), iptr(None), fptr(None), dtype)
        g = abi.PointMlpDgradArgs()
        g.dy, g.w, g.out, g.dtype = dy, _typed(b, t['w'], dtype), _typed_out(b, 'h.out', (M, K), dtype), dtype
        g.prev_y, g.prev_scale, g.prev_shift = xp, fptr(t['sc']), fptr(t['sh'])
        g.psum_dz, g.psum_dzy = fptr(b.out('h.psum_dz', (T, K))), fptr(b.out('h.psum_dzy', (T, K)))
        g.M, g.K, g.N, g.rows_per_frustum, g.arith = M, K, N, rpf, arith
        if pre:
            pf, pd, stride = x3_planes(env, t['w'])
            g.w_x3, g.w_x3_stride = pd.data_ptr(), stride
            b.keep += [pf, pd]
        w = abi.PointMlpWgradArgs(act, dy, fptr(b.out('h.slabs', (M // rps_, K, N))), M, K, N, rpf, rps_, arith)
        return 't3d_pointmlp_bwd', (g, w)
    host.query = lambda lib, args: lib.t3d_pointmlp_bwd_hosts_riders(C.byref(args[0]), C.byref(args[1]))
    host.tile = (tk, tn)
    return host


def _pool_inputs(M, K, N, rpf, seed):
    """tests/test_kernels_gpu.py `_pool_case`"""
    r = np.random.RandomState(seed)
    B = M // rpf
    d = dict(x=r.normal(size=(M, K)).astype(np.float32), sc=(0.5 + r.uniform(size=K)).astype(np.float32),
             sh=(r.normal(size=K) * 0.3).astype(np.float32), w=(r.normal(size=(K, N)) / np.sqrt(K)).astype(np.float32),
             bias=(r.normal(size=N) * 0.1).astype(np.float32), coef=r.normal(size=(3, N)).astype(np.float32),
             dpool=r.normal(size=(B, N)).astype(np.float32))
    d['sc'][::5] *= -1
    d['coef'][1] *= 1e-2
    d['coef'][2] *= 1e-3
    hot = r.randint(0, rpf, size=(B, 24))
    d['argidx'] = np.take_along_axis(hot, r.randint(0, 24, size=(B, N)), 1).astype(np.int32)
    d['argidx'][r.uniform(size=(B, N)) < 0.1] = -1
    d['argidx'][0, :N // 2] = 5
    d['g'] = (r.normal(size=(K, K))).astype(np.float32)
    d['abar'] = r.normal(size=K).astype(np.float32)
    d['p'] = (r.normal(size=(K, K)) / np.sqrt(K)).astype(np.float32)
    d['rc'] = r.normal(size=K).astype(np.float32)
    d['sm'] = (r.normal(size=(M, K)) * (r.uniform(size=(M, 1)) < 0.1)).astype(np.float32)
    return d


def stage1_host(env, M, K, N, rpf, arith, rps=None, dtype=abi.F32):
    """t3d_pool_bwd_stage1 (test_fused_pool_stages_equal_the_separate_launches' structs)."""
    d = _pool_inputs(M, K, N, rpf, M + K + N)
    p_rps, ptk, ptn = wgrad_tile(env.lib, M, K, K)
    if rps is None or rps == p_rps:      # csrc/pointmlp.hip gram_tile: square tiles only -- the plan's where it is 128 x 128 ...
        rps_, gt = p_rps, (128 if (ptk, ptn) == (128, 128) else 64)
    else:                                # ... and by shape where rows_per_split is not the plan's
        rps_, gt = rps, (128 if K % 128 == 0 else 64)
    if arith == X3:
        gt = 64                          # (x3: 64 x 64 tiles only)

    def host(b):
        t = {k: b.inp(d[k]) for k in ('x', 'sc', 'sh', 'w', 'bias', 'coef')}
        x = t['x']
        if dtype == abi.BF16:
            x = x.to(torch.bfloat16)
            b.keep.append(x)
        act = abi.ActSrc(C.cast(C.c_void_p(x.data_ptr()), abi.F), K, 0, fptr(t['sc']), fptr(t['sh']), 1, fptr(None), 0, dtype)
        nch = (N + 127) // 128
        ga = abi.PointMlpGramArgs(act, fptr(b.out('h.gram', (M // rps_, K, K))), M, K, rpf, rps_, arith)
        ca = abi.ActColsumArgs(act, M, K, rpf, fptr(b.out('h.abar', (M // 128, K))))
        qa = abi.PoolBwdPrepArgs(fptr(t['w']), fptr(t['bias']), fptr(t['coef']), K, N, fptr(b.out('h.p', (nch, K, K))), fptr(b.out('h.rc', (nch, K))),
                                 fptr(b.out('h.wc', (N, K))))
        return 't3d_pool_bwd_stage1', (ga, ca, qa)
    host.query = lambda lib, args: lib.t3d_pool_bwd_stage1_hosts_riders(*[C.byref(a) for a in args])
    host.tile = gt
    return host


def stage2_host(env, M, K, N, rpf, arith, dtype=abi.F32, live=False):
    """t3d_pool_bwd_stage2 (same test)."""
    d = _pool_inputs(M, K, N, rpf, M + K + N)

    def host(b):
        t = {k: b.inp(v) for k, v in d.items()}
        x = t['x']
        if dtype == abi.BF16:
            x = x.to(torch.bfloat16)
            b.keep.append(x)
        xp = C.cast(C.c_void_p(x.data_ptr()), abi.F)
        act = abi.ActSrc(xp, K, 0, fptr(t['sc']), fptr(t['sh']), 1, fptr(None), 0, dtype)
        f = abi.PoolWgradFinishArgs()
        f.a, f.argidx, f.dpool, f.coef, f.w, f.bias = act, iptr(t['argidx']), fptr(t['dpool']), fptr(t['coef']), fptr(t['w']), fptr(t['bias'])
        f.g, f.abar, f.B, f.K, f.N, f.rows_per_frustum, f.dw = fptr(t['g']), fptr(t['abar']), M // rpf, K, N, rpf, fptr(b.out('h.dw', (K, N)))
        dg = abi.PointMlpDgradGramArgs()
        dg.a, dg.p, dg.rowconst, dg.add_in, dg.prev_y, dg.prev_scale, dg.prev_shift = act, fptr(t['p']), fptr(t['rc']), fptr(t['sm']), xp, fptr(t['sc']), fptr(t['sh'])
        if live:      # the sparse rows with their row flags (what the one-pass form takes)
            dg.add_live = iptr(b.inp((np.abs(d['sm']).sum(1) > 0).astype(np.int32)))
        odt = torch.bfloat16 if dtype == abi.BF16 else torch.float32
        dg.out = C.cast(C.c_void_p(b.out('h.da', (M, K), odt).data_ptr()), abi.F)
        dg.psum_dz, dg.psum_dzy = fptr(b.out('h.psum_dz', (M // 128, K))), fptr(b.out('h.psum_dzy', (M // 128, K)))
        dg.M, dg.K, dg.rows_per_frustum, dg.dtype, dg.arith = M, K, rpf, dtype, arith
        return 't3d_pool_bwd_stage2', (f, dg)
    host.query = lambda lib, args: lib.t3d_pool_bwd_stage2_hosts_riders(*[C.byref(a) for a in args])
    return host


class Form:
    """One row of the table: kernel form, launcher family, builder + arguments, what the row claims about the dispatch."""

    def __init__(self, kernel, family, builder, kw, arith, gemm, claim='', env=None, unreachable=None, big=False):
        self.kernel, self.family, self.builder, self.kw, self.arith, self.gemm = kernel, family, builder, kw, arith, gemm
        self.claim, self.env, self.unreachable, self.big = claim, env or {}, unreachable, big

    @property
    def id(self):
        return self.kernel.replace(' ', '')

    def args_text(self):
        if self.unreachable:
            return 'none: ' + self.unreachable
        kw = dict(self.kw)
        s = ', '.join('%s=%s' % (k, kw[k]) for k in ('M', 'K', 'N', 'rpf') if k in kw)
        extra = [k if v is True else '%s=%s' % (k, v) for k, v in kw.items() if k not in ('M', 'K', 'N', 'rpf') and v not in (False, None)]
        extra += ['%s=%s' % kv for kv in self.env.items()]
        return s + ', arith=%s' % ('fp32_mfma' if self.arith == F32 else 'bf16x3') + (', ' + ', '.join(extra) if extra else '')


def _bwd_forms():
    rows = []
    # (DBN, tk, tn) -> shape.  Narrow (DBN = 64): M = 256 in ONE split, which is not t3d_wgrad_plan's split (128 rows), so the
    # fallback tile rule holds: tk = K > 64 ? 128 : 64, tn = N % 128 == 0 ? 128 : 64.  N outside {64, 128} keeps the one-pass form
    # away.  Wide (DBN = 128) needs K % 128 == 0 and (M / 128) * (K / 128) >= 512: K = 512 at M = 16384 with the plan's own split
    # and tile.
    shapes = {
        (64, 64, 64): dict(M=256, K=64, N=192, rpf=128, rps=256), (64, 64, 128): dict(M=256, K=64, N=256, rpf=128, rps=256),
        (64, 128, 64): dict(M=256, K=128, N=192, rpf=128, rps=256), (64, 128, 128): dict(M=256, K=128, N=256, rpf=128, rps=256),
        (128, 128, 64): dict(M=16384, K=512, N=192, rpf=1024, rps=None), (128, 128, 128): dict(M=16384, K=512, N=256, rpf=1024, rps=None),
        # the plan (not the fallback) gives 64 x 64 tiles for 128 -> 64 at M = 65536, and its split leaves too few workgroups for the
        # one-pass form
        (128, 64, 64): dict(M=65536, K=128, N=64, rpf=1024, rps=None),
    }
    for path, arith, pre in (('PathF32', F32, False), ('PathX3', X3, False), ('PathX3P', X3, True)):
        for dbn in (64, 128):
            for tk, tn in ((64, 64), (64, 128), (128, 64), (128, 128)):
                name = 'k_pointmlp_bwd_r<%d, %d, %d, %s>' % (dbn, tk, tn, path)
                if (dbn, tk, tn) == (128, 64, 128):
                    rows.append(Form(name, 'bwd', None, {}, arith, GEMM_BWD, unreachable='wide data-gradient tiles need K % 128 == 0; the fallback then '
                                     'gives tk = 128, and t3d_wgrad_plan prefers (128, 64) to (64, 128) whenever both divide (same tile count)'))
                    continue
                kw = dict(shapes[(dbn, tk, tn)], pre=pre)
                rows.append(Form(name, 'bwd', bwd_host, kw, arith, GEMM_BWD, claim=(dbn, tk, tn), big=dbn == 128))
    return rows


HOST_FORMS = [
    Form('k_pointmlp_fwd_r<64, false, PathF32>', 'fwd', fwd_host, dict(M=256, K=64, N=64, rpf=128), F32, GEMM_FWD, claim=64),
    Form('k_pointmlp_fwd_r<128, false, PathF32>', 'fwd', fwd_host, dict(M=32768, K=64, N=256, rpf=1024), F32, GEMM_FWD, claim=128, big=True),
    Form('k_pointmlp_fwd_r<64, true, PathF32>', 'fwd', fwd_host, dict(M=256, K=3, N=192, rpf=128, sub=True), F32, GEMM_FWD, claim=64),
    Form('k_pointmlp_fwd_r<128, true, PathF32>', 'fwd', fwd_host, dict(M=32768, K=3, N=256, rpf=128, sub=True), F32, GEMM_FWD, claim=128, big=True),
    Form('k_pointmlp_fwd_r<64, false, PathX3>', 'fwd', fwd_host, dict(M=256, K=64, N=64, rpf=128), X3, GEMM_FWD, claim=64),
    Form('k_pointmlp_fwd_r<128, false, PathX3>', 'fwd', fwd_host, dict(M=32768, K=64, N=256, rpf=1024), X3, GEMM_FWD, claim=128, big=True),
    Form('k_pointmlp_fwd_r<64, false, PathX3P>', 'fwd', fwd_host, dict(M=256, K=64, N=64, rpf=128, pre=True), X3, GEMM_FWD, claim=64),
    Form('k_pointmlp_fwd_r<128, false, PathX3P>', 'fwd', fwd_host, dict(M=32768, K=64, N=256, rpf=1024, pre=True), X3, GEMM_FWD, claim=128, big=True),
    Form('k_pointmlp_fwd_w8_r<256, PathX3W>', 'fwd', fwd_host, dict(M=256, K=64, N=256, rpf=128), X3, GEMM_FWD, claim=256, env={'T3D_X3_W8': '2'}),
    Form('k_pointmlp_fwd_w8_r<256, PathX3WP>', 'fwd', fwd_host, dict(M=256, K=64, N=256, rpf=128, pre=True), X3, GEMM_FWD, claim=256, env={'T3D_X3_W8': '2'}),
    Form('k_pointmlp_wgrad_r<64, 64, false>', 'wgrad', wgrad_host, dict(M=512, K=32, N=192, rpf=128), F32, GEMM_WGRAD, claim=(64, 64)),
    Form('k_pointmlp_wgrad_r<64, 64, true>', 'wgrad', wgrad_host, dict(M=512, K=3, N=192, rpf=128, sub=True), F32, GEMM_WGRAD, claim=(64, 64)),
] + _bwd_forms() + [
    Form('k_pool_bwd_stage1_r<64, PathF32>', 'stage1', stage1_host, dict(M=512, K=64, N=256, rpf=128), F32, GEMM_GRAM, claim=64),
    Form('k_pool_bwd_stage1_r<128, PathF32>', 'stage1', stage1_host, dict(M=512, K=128, N=256, rpf=128, rps=256), F32, GEMM_GRAM, claim=128),
    Form('k_pool_bwd_stage1_r<64, PathX3>', 'stage1', stage1_host, dict(M=512, K=64, N=256, rpf=128), X3, GEMM_GRAM, claim=64),
    Form('k_pool_bwd_stage2_r<64, PathF32>', 'stage2', stage2_host, dict(M=512, K=128, N=256, rpf=128), F32, GEMM_DGRAD_GRAM, claim=64),
    Form('k_pool_bwd_stage2_r<128, PathF32>', 'stage2', stage2_host, dict(M=32768, K=256, N=256, rpf=1024), F32, GEMM_DGRAD_GRAM, claim=128, big=True),
    Form('k_pool_bwd_stage2_r<64, PathX3>', 'stage2', stage2_host, dict(M=512, K=128, N=256, rpf=128), X3, GEMM_DGRAD_GRAM, claim=64),
    Form('k_pool_bwd_stage2_r<128, PathX3>', 'stage2', stage2_host, dict(M=32768, K=256, N=256, rpf=1024), X3, GEMM_DGRAD_GRAM, claim=128, big=True),
]

# D. forms that do not host: the `_r` call runs the set as a launch of its own in front of (or behind) the GEMM
NON_HOSTING = [      # (name, builder, arguments, arith, FakeLib can run it: the specification library has no bf16)
    ('fp32 register forward (K <= 4, N in {64, 128})', fwd_host, dict(M=256, K=3, N=64, rpf=128, sub=True), F32, True),
    ('k_pointmlp_fwd_pool (pooled layer without an output tensor, K = 128)', fwd_host, dict(M=256, K=128, N=256, rpf=128, nostore_pool=True), F32, True),
    ('one-pass fused backward (K, N in {64, 128})', bwd_host, dict(M=256, K=64, N=64, rpf=128), F32, True),
    ('x3 weight gradient', wgrad_host, dict(M=512, K=64, N=192, rpf=128), X3, True),
    ('register weight gradient (K <= 4, N in {64, 128})', wgrad_host, dict(M=512, K=3, N=64, rpf=128, sub=True), F32, True),
    ('128-wide weight-gradient tiles', wgrad_host, dict(M=512, K=128, N=256, rpf=128, rps=256), F32, True),
    ('bf16 forward', fwd_host, dict(M=256, K=64, N=64, rpf=128, dtype=abi.BF16), abi.ARITH_AUTO, False),
    ('bf16 weight gradient', wgrad_host, dict(M=512, K=64, N=192, rpf=128, dtype=abi.BF16), abi.ARITH_AUTO, False),
    ('bf16 fused backward, split form', bwd_host, dict(M=256, K=64, N=192, rpf=128, dtype=abi.BF16), abi.ARITH_AUTO, False),
    ('bf16 fused backward, one-pass form', bwd_host, dict(M=256, K=64, N=64, rpf=128, dtype=abi.BF16), abi.ARITH_AUTO, False),
    ('bf16 pooled stage 1, split form (K = 64)', stage1_host, dict(M=512, K=64, N=256, rpf=128, dtype=abi.BF16), abi.ARITH_AUTO, False),
    ('k_pool_bwd_stage1_h (bf16, K = 128)', stage1_host, dict(M=512, K=128, N=256, rpf=128, rps=128, dtype=abi.BF16), abi.ARITH_AUTO, False),
    ('bf16 pooled stage 2, split form (K = 128)', stage2_host, dict(M=512, K=128, N=256, rpf=128, dtype=abi.BF16), abi.ARITH_AUTO, False),
    ('k_pool_bwd_stage2_h (bf16, K = 256, sparse rows with row flags)', stage2_host, dict(M=512, K=256, N=256, rpf=128, dtype=abi.BF16, live=True), abi.ARITH_AUTO, False),
]


def forms_markdown():
    """The table of DESIGN.md (tools/rider_forms_table.py)."""
    out = ['| rider form | launcher | smallest selecting arguments |', '|---|---|---|']
    for f in HOST_FORMS:
        out.append('| `%s` | `t3d_%s_r` | %s |' % (f.kernel, {'fwd': 'pointmlp_fwd', 'wgrad': 'pointmlp_wgrad', 'bwd': 'pointmlp_bwd', 'stage1': 'pool_bwd_stage1',
                                                             'stage2': 'pool_bwd_stage2'}[f.family], f.args_text()))
    out += ['', 'Forms that do not host (the set runs as a launch of its own beside the GEMM):', '']
    for row in NON_HOSTING:
        out.append('* %s' % row[0])
    return '\n'.join(out) + '\n'


# ---- checks shared by the two test files ------------------------------------------------------------------------------------------------
def check_wide_rider(env, M, K, N, rpf):
    """The wide rider as a set of its own.  N = 1024 (the first shape of the stand-alone test) needs 80.5 KB of LDS: refused by the
    76 KB rule, and run here at N = 512 instead."""
    if sparse_rows_lds(N) > 76 * 1024:
        ops = pool_bwd_mid_case(M, K, N, rpf)(Bufs(env.dev))
        make_set(env, ops, plan_rc=ERR_SHAPE)
        N = 512
    rs = check_set_alone(env, pool_bwd_mid_case(M, K, N, rpf), what='pool_bwd_mid M=%d K=%d N=%d' % (M, K, N))
    assert rs.n_wg == mid_blocks(M, K) and rs.n_wg > RIDER_MAX_WG, rs.n_wg      # one workgroup per block, not the 32 of a set with barriers
    assert rs.lds_bytes == sparse_rows_lds(N), rs.lds_bytes


def small_chain_case():
    """A cheap dependent two-op set (3 blocks, then 1) for the non-hosting forms and the refusals."""
    return fc_chain_case(32, (64, 96, 32), seed=5, tag='s')


_SET_REF = {}


def set_reference(env, key, case, depends=None):
    """Stand-alone launches and the set alone, compared once per library and shared by every host row."""
    k = (id(env.lib), key)
    if k not in _SET_REF:
        n = len(case(Bufs(env.dev)))
        depends = default_depends(n) if depends is None else depends
        apart = run_apart(env, case)
        alone, _, words = run_alone(env, case, depends)
        check_guards(alone, key + ' set alone')
        assert_same_bits(apart, alone, key + ': set alone vs stand-alone launches')
        check_sync_words(words, depends, REPS, key + ' (alone)')
        _SET_REF[k] = alone
    return _SET_REF[k]


def check_non_hosting(env, name, expect_query=None):
    """The `_r` call with a set on a form that has no rider kernel: the bytes of the set, then the host."""
    _, builder, kw, arith, _ = [n for n in NON_HOSTING if n[0] == name][0]
    host = builder(env, arith=arith, **kw)
    if expect_query is not None:
        _, args = host(Bufs(env.dev))
        assert host.query(env.lib, args) == expect_query, name
    check_hosted(env, host, small_chain_case(), name, set_ref=set_reference(env, 'small chain', small_chain_case()))


def form_host(env, form):
    return form.builder(env, arith=form.arith, **form.kw)


def check_form_claims(env, form, host):
    """The row's reading of the dispatch, asked of the library: it hosts, with the arithmetic and the tiles the row names."""
    kw = form.kw
    _, args = host(Bufs(env.dev))
    assert host.query(env.lib, args) == 1, '%s: the launcher does not host these arguments' % form.kernel
    n_arith = kw['K'] if form.family in ('stage1', 'stage2') else kw['N']
    assert env.lib.t3d_gemm_arithmetic(form.arith, abi.F32, kw['K'], n_arith, form.gemm) == form.arith or kw.get('sub'), form.kernel
    if form.family == 'fwd':
        got = 256 if form.env.get('T3D_X3_W8') == '2' and kw['N'] % 256 == 0 else (128 if fwd_wide(kw['M'], kw['N']) else 64)
    elif form.family == 'wgrad':
        got = host.tile
    elif form.family == 'bwd':
        got = (128 if dgrad_wide(kw['M'], kw['K']) else 64,) + tuple(host.tile)
    elif form.family == 'stage1':
        got = host.tile
    else:
        got = 128 if dgrad_gram_wide(kw['M'], kw['K']) else 64
    assert got == form.claim, '%s: these arguments select tiles %s' % (form.kernel, got)


def check_form(env, form):
    host = form_host(env, form)
    check_form_claims(env, form, host)
    case = fc_chain_case(**FC_CHAIN)
    return check_hosted(env, host, case, form.kernel, set_ref=set_reference(env, 'fc chain', case))


def check_form_with_wide_rider(env, form):
    """The wide rider inside a host: more rider workgroups than the host has tiles of its own (the small rows), and more LDS than the
    host asks for (`lds_with` takes the rider's)."""
    host = form_host(env, form)
    check_form_claims(env, form, host)
    M, K, N, rpf = 256, 256, 512, 128
    case = pool_bwd_mid_case(M, K, N, rpf)
    rs = check_hosted(env, host, case, form.kernel + ' + pool_bwd_mid', depends=[0], set_ref=set_reference(env, 'mid', case, [0]))
    assert rs.n_wg == mid_blocks(M, K) and rs.lds_bytes == sparse_rows_lds(N)
    return rs


def _fc_op(B=32, N=64, K=64):
    b = Bufs(torch.device('cpu'))
    a, _ = fc_fwd_args(b, b.inp(np.zeros((B, K), np.float32)), K, N, B, np.random.RandomState(0), True, False)
    a._keep = b
    return a


def _plan(env, ops, n_ops=None, kinds=None):
    rs = abi.RiderSet()
    for k, (name, arg) in enumerate(ops):
        rs.ops[k] = small_op(name, arg, depends=int(k > 0))
        if kinds is not None:
            rs.ops[k].kind = kinds[k]
    rs.n_ops = len(ops) if n_ops is None else n_ops
    return env.lib.t3d_riders_plan(C.byref(rs))


def check_plan_refusals(env):
    fc = ('t3d_fc_fwd', _fc_op())
    assert _plan(env, [fc]) == 0
    assert _plan(env, [fc], n_ops=0) == ERR_ARG
    assert _plan(env, [fc] * abi.RIDER_MAX_OPS) == 0
    assert _plan(env, [fc] * abi.RIDER_MAX_OPS, n_ops=abi.RIDER_MAX_OPS + 1) == ERR_ARG
    assert _plan(env, [fc], kinds=[0]) == ERR_ARG
    assert _plan(env, [fc], kinds=[8]) == ERR_ARG
    assert _plan(env, [('t3d_fc_fwd', _fc_op(B=33))]) == ERR_SHAPE
    cpu = lambda: Bufs(torch.device('cpu'))
    (_, bwd), = fc_bwd_case(33, 64, 64, True, False)(cpu())
    assert _plan(env, [('t3d_fc_bwd', bwd)]) == ERR_SHAPE
    (_, din), = fc_dinput_case(33, 64, 64, False)(cpu())
    assert _plan(env, [('t3d_fc_dinput', din)]) == ERR_SHAPE
    (_, f), = bn_fwd_case(16, 8, False)(cpu())
    assert _plan(env, [('t3d_bn_fwd_finalize', f)]) == 0
    f.n_tiles = 512
    assert _plan(env, [('t3d_bn_fwd_finalize', f)]) == 0
    f.n_tiles = 513
    assert _plan(env, [('t3d_bn_fwd_finalize', f)]) == ERR_SHAPE
    (_, g), = bn_bwd_case(16, 8, True)(cpu())
    assert _plan(env, [('t3d_bn_bwd_finalize', g)]) == 0
    g.n_tiles = 513
    assert _plan(env, [('t3d_bn_bwd_finalize', g)]) == ERR_SHAPE
    g.n_tiles, g.coef = 8, None
    assert _plan(env, [('t3d_bn_bwd_finalize', g)]) == ERR_SHAPE
    (mid,) = pool_bwd_mid_case(256, 256, 512, 128)(cpu())
    assert _plan(env, [mid]) == 0
    assert _plan(env, [mid, fc]) == ERR_ARG
    assert _plan(env, [fc, mid]) == ERR_ARG
    (mid1k,) = pool_bwd_mid_case(512, 128, 1024, 256)(cpu())
    assert _plan(env, [mid1k]) == ERR_SHAPE


# the smallest hosting row of each launcher family (fp32-MFMA)
FAMILY_ROWS = ['k_pointmlp_fwd_r<64, false, PathF32>', 'k_pointmlp_wgrad_r<64, 64, false>', 'k_pointmlp_bwd_r<64, 64, 64, PathF32>',
               'k_pool_bwd_stage1_r<64, PathF32>', 'k_pool_bwd_stage2_r<64, PathF32>']


def form_by_name(kernel):
    return [f for f in HOST_FORMS if f.kernel == kernel][0]


def _untouched(b, what):
    for k, (f, n, pre) in b.snapshot().items():
        if not pre:
            assert (f == SENT).all(), '%s: %s was written by a refused call' % (what, k)


def check_launch_refusals(env):
    """t3d_run_riders and every `_r` launcher: a set without barrier words, with 0 or 33 workgroups for two ops, or with a negative
    LDS size is T3D_ERR_ARG, and nothing runs."""
    def bad_sets(b):
        ops = small_chain_case()(b)
        for what, mutate in (('sync = NULL', lambda r: setattr(r, 'sync', None)), ('n_wg = 33', lambda r: setattr(r, 'n_wg', 33)),
                             ('n_wg = 0', lambda r: setattr(r, 'n_wg', 0)), ('lds_bytes = -1', lambda r: setattr(r, 'lds_bytes', -1))):
            rs, _ = make_set(env, ops)
            assert rs.n_ops == 2
            mutate(rs)
            yield what, rs

    for what, rs in bad_sets(Bufs(env.dev)):
        assert env.lib.t3d_run_riders(C.byref(rs), env.stream()) == ERR_ARG, what
    assert env.lib.t3d_run_riders(None, env.stream()) == ERR_ARG
    for kernel in FAMILY_ROWS:
        form = form_by_name(kernel)
        b = Bufs(env.dev)
        fn, args = form_host(env, form)(b)
        for what, rs in bad_sets(b):
            rc = getattr(env.lib, fn + '_r')(*[C.byref(a) for a in args], C.byref(rs), env.stream())
            assert rc == ERR_ARG, (fn, what, rc)
        env.sync()
        _untouched(b, fn + '_r')


def check_query_refusals(env):
    """Each `_hosts_riders` query answers with the launcher's own error code for arguments the launcher rejects."""
    for kernel in FAMILY_ROWS:
        form = form_by_name(kernel)
        host = form_host(env, form)
        for what, want in (('null', ERR_ARG), ('shape', ERR_SHAPE)):
            _, args = host(Bufs(env.dev))
            assert host.query(env.lib, args) >= 0, kernel      # (1 on the device library: check_form_claims)
            a = args[0]
            if form.family == 'fwd':
                if what == 'null': a.w = None
                else: a.M += 64
            elif form.family == 'wgrad':
                if what == 'null': a.slabs = None
                else: a.rows_per_split = 384
            elif form.family == 'bwd':
                if what == 'null': a.w = None
                else: args[1].M *= 2
            elif form.family == 'stage1':
                if what == 'null': a.slabs = None
                else: a.rows_per_split = 384
            else:
                if what == 'null': args[1].out = None
                else: args[1].rows_per_frustum = 384
            assert host.query(env.lib, args) == want, (kernel, what)
