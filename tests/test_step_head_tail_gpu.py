"""GPU: the merged launches at the two ends of a training step against the launches they stand for, bit for bit.

  t3d_step_head          = t3d_schedule_step, t3d_split_x3_frag, t3d_pointmlp_fwd (first layer: the fp32 register kernel)
  t3d_reduce_slabs_adam  = t3d_reduce_slabs, t3d_adam_tf_step

and the step program (step.TrainStep) with the merged launches against the same program without them."""
import ctypes as C

import numpy as np
import pytest
import torch

from transferable3d_amd import abi
from transferable3d_amd.abi import fptr

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- head ---------------------------------------------------------------------------------------------------------------------------
def _head_state(n_out, step0, seed=7):
    """B=2, N=128 points, C=4: the raw batch, a parameter buffer with the first layer's [4, n_out] matrix and bias and two x3 layers
    (64 x 64 and 64 x 128, both arrangements) in the fragment table, the plane buffers, the schedule words."""
    r = np.random.RandomState(seed)
    dev = torch.device('cuda')
    B, N, Cc = 2, 128, 4
    M = B * N
    off_w1, off_b1 = 0, 4 * n_out
    off_a = (off_b1 + n_out + 7) // 8 * 8 + 8          # (a gap in front of, between and behind the x3 matrices)
    off_b = off_a + 64 * 64 + 16
    n_par = off_b + 64 * 128 + 24
    stride = (n_par + 7) // 8 * 8
    t = dict(pc=torch.as_tensor(r.normal(size=(M, Cc)).astype(np.float32)).to(dev),
             params=torch.as_tensor(r.normal(size=n_par).astype(np.float32)).to(dev),
             pf=torch.full((3 * stride,), 7.0, dtype=torch.bfloat16, device=dev),
             pd=torch.full((3 * stride,), 7.0, dtype=torch.bfloat16, device=dev),
             y=torch.zeros(M, n_out, device=dev), psum=torch.zeros(M // 128, n_out, device=dev),
             psumsq=torch.zeros(M // 128, n_out, device=dev), hyper=torch.tensor([step0, 0.0, 0.5, 0.0], device=dev))
    raw, nblk = abi.x3_frag_table([(off_a, 64, 64), (off_b, 64, 128)])
    t['tab'] = torch.from_numpy(raw).to(dev)
    a = abi.PointMlpFwdArgs()
    a.a = abi.ActSrc(fptr(t['pc']), Cc, 0, fptr(None), fptr(None), 0, fptr(None), 0, abi.F32)
    a.w, a.bias, a.y = fptr(t['params'][off_w1:]), fptr(t['params'][off_b1:]), fptr(t['y'])
    a.psum, a.psumsq = fptr(t['psum']), fptr(t['psumsq'])
    a.M, a.K, a.N, a.rows_per_frustum, a.dtype, a.arith = M, Cc, n_out, N, abi.F32, abi.ARITH_BF16X3
    return t, a, nblk, stride


@pytest.mark.parametrize('n_out', [64, 128])
@pytest.mark.parametrize('step0', [0.0, 25000.0])      # 25000 steps of 32 = 800000 samples: past the first learning-rate decay boundary
def test_step_head_equals_its_three_launches(hip_lib, n_out, step0):
    sched = abi.Schedule(1e-3, 0.5, 800000.0, 0.5, 0.5, 800000.0, 0.99, 0.9, 0.999, 32, 0)
    s = _stream()
    out = {}
    for mode in ('apart', 'fused'):
        t, a, nblk, stride = _head_state(n_out, step0)
        planes = (fptr(t['params']), C.c_void_p(t['pf'].data_ptr()), C.c_void_p(t['pd'].data_ptr()), stride, C.c_void_p(t['tab'].data_ptr()), 2, nblk)
        for _ in range(2):                              # two steps: the second starts from the first one's schedule words
            if mode == 'apart':
                assert hip_lib.t3d_schedule_step(fptr(t['hyper']), C.byref(sched), s) == 0
                assert hip_lib.t3d_split_x3_frag(*planes, s) == 0
                assert hip_lib.t3d_pointmlp_fwd(C.byref(a), s) == 0
            else:
                assert hip_lib.t3d_step_head(C.byref(a), *planes, fptr(t['hyper']), C.byref(sched), s) == 0
        torch.cuda.synchronize()
        out[mode] = t
    assert float(out['apart']['hyper'][0]) == step0 + 2.0
    if step0 > 0:
        assert abs(float(out['apart']['hyper'][1]) - 5e-4) < 1e-9
    assert float(out['apart']['y'].abs().sum()) > 0 and not torch.equal(out['apart']['pf'], torch.full_like(out['apart']['pf'], 7.0))
    for k in ('hyper', 'pf', 'pd', 'y', 'psum', 'psumsq'):      # (pf / pd: the whole buffers, all three planes and the gaps)
        assert torch.equal(out['apart'][k], out['fused'][k]), k


def test_step_head_refuses_a_layer_the_register_kernel_does_not_take(hip_lib):
    t, a, nblk, stride = _head_state(64, 0.0)
    sched = abi.Schedule(1e-3, 0.5, 800000.0, 0.5, 0.5, 800000.0, 0.99, 0.9, 0.999, 32, 0)
    planes = (fptr(t['params']), C.c_void_p(t['pf'].data_ptr()), C.c_void_p(t['pd'].data_ptr()), stride, C.c_void_p(t['tab'].data_ptr()), 2, nblk)
    a.dtype = abi.BF16
    assert hip_lib.t3d_step_head(C.byref(a), *planes, fptr(t['hyper']), C.byref(sched), _stream()) == -1      # T3D_ERR_ARG
    assert hip_lib.t3d_step_head_takes(C.byref(a)) == 0
    a.dtype = abi.F32
    assert hip_lib.t3d_step_head_takes(C.byref(a)) == 1
    assert hip_lib.t3d_step_head(C.byref(a), *planes, fptr(None), C.byref(sched), _stream()) == -1
    # an input that is not raw (a scale / shift or a per-frustum offset some launch would have to write first) is not a head layer
    a.a.scale, a.a.shift = fptr(t['psum']), fptr(t['psumsq'])
    assert hip_lib.t3d_step_head_takes(C.byref(a)) == 0
    assert hip_lib.t3d_step_head(C.byref(a), *planes, fptr(t['hyper']), C.byref(sched), _stream()) == -1
    a.a.scale, a.a.shift, a.a.sub, a.a.sub_ld = fptr(None), fptr(None), fptr(t['psum']), 4
    assert hip_lib.t3d_step_head(C.byref(a), *planes, fptr(t['hyper']), C.byref(sched), _stream()) == -1
    a.a.sub, a.a.sub_ld = fptr(None), 0
    a.K, a.a.ldx = 8, 8                                  # not the register kernel's layer
    assert hip_lib.t3d_step_head_takes(C.byref(a)) == 0
    torch.cuda.synchronize()
    assert float(t['hyper'][0]) == 0.0 and float(t['y'].abs().sum()) == 0.0


# ---- tail ---------------------------------------------------------------------------------------------------------------------------
def test_reduce_slabs_adam_equals_reduction_then_adam_over_three_steps(hip_lib):
    """Three slab tensors (2, 3 and 48 slabs; 67 elements is no multiple of 4: the reducer's scalar path) with gaps of directly written
    gradients in front of, between and behind them; 48 slabs walk the 32-slab and the 8-slab loops, 640 elements more than one block."""
    r = np.random.RandomState(11)
    dev = torch.device('cuda')
    sizes = [(2, 640), (3, 67), (48, 1536)]             # (slabs, elements)
    gaps = [12, 1100, 5, 333]                           # 1100: more than one workgroup of a range
    table, tensors = (abi.SlabDesc * 3)(), []
    so, go = 0, gaps[0]
    for i, (ns, ne) in enumerate(sizes):
        table[i] = abi.SlabDesc(so, go, ne, ns)
        tensors.append((go, ne))
        so += (ns * ne + 3) // 4 * 4                   # (16-byte aligned slab regions: the 2- and 48-slab tensors take the float4 path)
        go += ne + gaps[i + 1]
    n = go
    ranges, nblk = abi.adam_range_table(n, tensors)
    assert [(o, k) for o, k, _ in ranges] == [(0, 12), (652, 1100), (1819, 5), (3360, 333)] and nblk == 5
    host = (abi.AdamRange * len(ranges))(*[abi.AdamRange(o, k, b, 0) for o, k, b in ranges])
    tab = torch.as_tensor(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
    rtab = torch.as_tensor(np.frombuffer(bytes(host), dtype=np.uint8).copy()).to(dev)
    tabp, rtabp = C.cast(C.c_void_p(tab.data_ptr()), C.POINTER(abi.SlabDesc)), C.cast(C.c_void_p(rtab.data_ptr()), C.POINTER(abi.AdamRange))
    covered = torch.zeros(n, dtype=torch.bool)
    for o, k in tensors:
        covered[o:o + k] = True
    w0 = r.normal(size=n).astype(np.float32)
    sched = abi.Schedule(1e-3, 0.5, 800000.0, 0.5, 0.5, 800000.0, 0.99, 0.9, 0.999, 32, 0)
    s = _stream()
    out = {}
    for mode in ('apart', 'fused'):
        rs = np.random.RandomState(12)
        w, m, v = torch.as_tensor(w0.copy()).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        g = torch.zeros(n, device=dev)
        hyper = torch.tensor([0.0, 0.0, 0.5, 0.0], device=dev)
        per_step = []
        for it in range(3):
            slab = torch.as_tensor((rs.normal(size=so) * 1e-2).astype(np.float32)).to(dev)
            direct = torch.as_tensor((rs.normal(size=n) * 1e-2).astype(np.float32)).to(dev)
            g.copy_(torch.where(covered.to(dev), g, direct))      # the directly written gradients of this step; stale sums where slabs reduce
            assert hip_lib.t3d_schedule_step(fptr(hyper), C.byref(sched), s) == 0
            if mode == 'apart':
                assert hip_lib.t3d_reduce_slabs(fptr(slab), fptr(g), tabp, 3, 1536, s) == 0
                assert hip_lib.t3d_adam_tf_step(fptr(w), fptr(g), fptr(m), fptr(v), n, fptr(hyper), 0.9, 0.999, 1e-8, 0.5, s) == 0
            else:
                assert hip_lib.t3d_reduce_slabs_adam(fptr(slab), fptr(g), tabp, 3, 1536, fptr(w), fptr(m), fptr(v), rtabp, len(ranges), nblk,
                                                     fptr(hyper), 0.9, 0.999, 1e-8, 0.5, s) == 0
            torch.cuda.synchronize()
            per_step.append([x.clone() for x in (w, m, v, g)])
        out[mode] = per_step
    assert not torch.equal(out['apart'][2][0], torch.as_tensor(w0).to(dev))
    for it in range(3):
        for k, name in enumerate(('params', 'm', 'v', 'grads')):
            assert torch.equal(out['apart'][it][k], out['fused'][it][k]), (it, name)


def test_adam_range_table_refuses_overlapping_slab_tensors():
    with pytest.raises(abi.T3DError):
        abi.adam_range_table(100, [(0, 40), (32, 16)])
    with pytest.raises(abi.T3DError):
        abi.adam_range_table(100, [(90, 16)])
    assert abi.adam_range_table(64, [(0, 64)]) == ([], 0)


# ---- program ------------------------------------------------------------------------------------------------------------------------
def test_three_steps_of_model_a_with_and_without_the_merged_launches(hip_lib):
    from transferable3d_amd.engine import Runtime
    from transferable3d_amd.step import build_training_step
    from transferable3d_amd.synthetic import make_batch
    B, N, Cc = 4, 128, 4
    out = {}
    for fuse in (False, True):
        g, model, step, loss = build_training_step(Runtime(lib=hip_lib), 'A', B, N, Cc, seed=5, use_hip_graph=True, fuse_head_tail=fuse)
        losses = []
        for k in range(3):                              # eager, capture + replay, replay
            model.inputs.load(make_batch(B, N, Cc, seed=40 + k))
            step.run()
            losses.append(float(loss))
        torch.cuda.synchronize()
        vs = g.vars
        names = [c[0] for kind, x in step.cache[True]['prog'] if kind == 'run' for c in x.calls if c[0].startswith('t3d')]
        out[fuse] = dict(loss=losses, params=vs.params[:vs.used].clone(), m=vs.adam_m[:vs.used].clone(), v=vs.adam_v[:vs.used].clone(),
                         grads=vs.grads[:vs.used].clone(), state=vs.state[:vs.state_used].clone(), hyper=g.hyper.clone(), names=names,
                         fused=list(step.fused))
    assert out[False]['fused'] == [] and out[True]['fused'] == ['t3d_step_head', 't3d_reduce_slabs_adam']
    assert len(out[False]['names']) - len(out[True]['names']) == 3
    assert out[True]['names'][0] == 't3d_step_head' and out[True]['names'][-1] == 't3d_reduce_slabs_adam'
    assert not any(n in out[True]['names'] for n in ('t3d_schedule_step', 't3d_split_x3_frag', 't3d_reduce_slabs', 't3d_adam_tf_step'))
    assert out[False]['loss'] == out[True]['loss'] and all(np.isfinite(out[True]['loss']))
    for k in ('params', 'm', 'v', 'grads', 'state', 'hyper'):
        assert torch.equal(out[False][k], out[True][k]), k
