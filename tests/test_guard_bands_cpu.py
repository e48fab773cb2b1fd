"""The guard-band harness (tests/guard_bands.py) is not vacuous: with torch ops standing in for a kernel, its checker fails for a
store one element before the interior, one element after it, a store into a row's padding, an unwritten element and a result that
consumed a band value -- each naming the operand -- and passes a clean op."""
import pytest
import torch

from guard_bands import G, INT64_BAND, INT_BAND, assert_clean, guarded, roundup4

DTYPES = [torch.float32, torch.bfloat16]


def _kernel(xc, K, coff, out_valid, over=0):
    """y = 2 * x[:, coff : coff + K]; `over` > 0 also reads that many columns past the valid ones and "masks" them.  Addresses the
    flat allocation from the ABI pointer, as a kernel does."""
    rows, ld = xc.view.shape
    flat = xc.buf
    idx = (G + torch.arange(rows)[:, None] * ld + coff + torch.arange(K + over)[None, :]).reshape(-1)
    a = flat[idx].reshape(rows, K + over).float()
    res = 2 * a[:, :K]
    if over:
        res[:, :over] += 0 * a[:, K:]          # "masked" with a multiply: NaN * 0 is still NaN
    out_valid.copy_(res.to(out_valid.dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_clean_op_passes(dtype):
    x = torch.randn(8, 12)
    xv, xc = guarded((8, 12), dtype, 'cpu', ld=24, col0=4, fill=x, name='x')
    yv, yc = guarded((8, 12), dtype, 'cpu', ld=20, name='y')
    assert xv.shape == (8, 24) and yv.shape == (8, 20) and xc.buf.numel() == 2 * G + 8 * 24
    assert torch.isnan(xc.buf[:G]).all() and torch.isnan(xc.buf[-G:]).all() and torch.isnan(xv[:, :4]).all() and torch.isnan(xv[:, 16:]).all()
    assert torch.equal(xc.valid, x.to(dtype))
    _kernel(xc, 12, 4, yc.valid)
    xc()
    yc(written=True)
    assert_clean('y', yc.valid, 2 * x.double())
    assert torch.equal(yc.valid.float(), (2 * x.to(dtype).float()).to(dtype).float())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('where', ['before', 'after'])
def test_store_outside_the_interior_fails(dtype, where):
    yv, yc = guarded((4, 8), dtype, 'cpu', name='psum')
    yv.fill_(1.0)
    yc(written=True)
    yc.buf[G - 1 if where == 'before' else G + 32] = 0.0
    with pytest.raises(AssertionError, match='psum: 1 store.s. %s the operand, nearest 1 element' % where.upper()):
        yc()


def test_store_into_row_padding_fails():
    yv, yc = guarded((4, 8), torch.float32, 'cpu', ld=12, name='out')
    yc.valid.fill_(1.0)
    yc(written=True)
    yv[2, 8] = 3.0
    with pytest.raises(AssertionError, match='out: 1 store.s. into the row PADDING'):
        yc()


def test_unwritten_element_fails_only_when_the_contract_says_whole_tensor():
    yv, yc = guarded((4, 8), torch.bfloat16, 'cpu', name='y')
    yv[:, :7] = 1.0
    yc()
    with pytest.raises(AssertionError, match='y: 4 element.s. never written'):
        yc(written=True)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('over', [1, 4])
def test_result_that_consumed_a_band_value_fails(dtype, over):
    """the stand-in reads `over` columns past the valid ones (row padding; on the last row with ld == width, the back band)"""
    x = torch.randn(8, 12)
    for ld in (24, 12):
        xv, xc = guarded((8, 12), dtype, 'cpu', ld=ld, fill=x, name='x')
        yv, yc = guarded((8, 12), dtype, 'cpu', name='y')
        _kernel(xc, 12, 0, yc.valid, over=over)
        xc()
        yc(written=True)
        with pytest.raises(AssertionError, match='y: %d non-finite' % (8 * over if ld == 24 else over)):
            assert_clean('y', yc.valid, 2 * x.double())


def test_integer_bands_and_modified_input():
    idx = torch.randint(0, 100, (3, 16), dtype=torch.int32)
    iv, ic = guarded((3, 16), torch.int32, 'cpu', fill=idx, name='argidx')
    assert (ic.buf[:G] == INT_BAND).all() and (ic.buf[-G:] == INT_BAND).all() and torch.equal(iv, idx)
    ic()
    iv[1, 1] += 1
    with pytest.raises(AssertionError, match='argidx: the launch changed an INPUT'):
        ic()
    ov, oc = guarded((3, 16), torch.int32, 'cpu', name='pamax')
    ov.copy_(idx)
    oc(written=True)
    oc.buf[-1] = 5
    with pytest.raises(AssertionError, match='pamax: 1 store.s. AFTER the operand, nearest %d element' % G):
        oc()


def test_fp64_operands_have_a_payload_sentinel_and_nan_bands():
    """the frustum ABI's fp64 operands: the same five failures, and a canonical NaN stored by the op is a store, not the sentinel"""
    x = torch.randn(5, 6, dtype=torch.float64)
    xv, xc = guarded((5, 6), torch.float64, 'cpu', fill=x, name='points')
    assert xv.dtype == torch.float64 and torch.isnan(xc.buf[:G]).all() and torch.isnan(xc.buf[-G:]).all() and torch.equal(xv, x)
    yv, yc = guarded((5, 6), torch.float64, 'cpu', name='out_points')
    assert torch.isnan(yc.buf).all() and (yc.buf.view(torch.int64) != torch.tensor(float('nan'), dtype=torch.float64).view(torch.int64)).all()
    with pytest.raises(AssertionError, match='out_points: 30 element.s. never written'):
        yc(written=True)
    yc(written=None)
    yv.copy_(2 * x)
    yv[4, 5] = float('nan')
    xc()
    yc(written=True)
    with pytest.raises(AssertionError, match='out_points: 30 element.s. written by a launch that must not touch it'):
        yc(written=None)
    with pytest.raises(AssertionError, match='out_points: 1 non-finite'):
        assert_clean('out_points', yv, 2 * x)
    for at, where in ((G - 1, 'BEFORE'), (G + 30, 'AFTER')):
        keep = yc.buf[at].clone()
        yc.buf[at] = 0.0
        with pytest.raises(AssertionError, match='out_points: 1 store.s. %s the operand, nearest 1 element' % where):
            yc()
        yc.buf[at] = keep                   # the payload survives a copy
        yc()
    xv[0, 0] += 1
    with pytest.raises(AssertionError, match='points: the launch changed an INPUT'):
        xc()


def test_int64_operands_and_a_uint64_scratch_through_an_int64_view():
    off = torch.tensor([0, 3, 3, 1 << 40], dtype=torch.int64)
    ov, oc = guarded((4,), torch.int64, 'cpu', fill=off, name='scene_offsets')
    assert (oc.buf[:G] == INT64_BAND).all() and (oc.buf[-G:] == INT64_BAND).all() and torch.equal(ov, off)
    oc()
    ov[3] -= 1
    with pytest.raises(AssertionError, match='scene_offsets: the launch changed an INPUT'):
        oc()
    mv, mc = guarded((7,), torch.int64, 'cpu', name='masks')          # uint64 bit masks: every pattern but the sentinel is a value
    mc(written=None)
    mv[:6] = torch.tensor([0, -1, 1, INT64_BAND, 2 ** 63 - 1, 5], dtype=torch.int64)        # 0, ~0, 1, 1 << 63, ...
    mc()
    with pytest.raises(AssertionError, match='masks: 1 element.s. never written'):
        mc(written=True)
    mc.buf[G + 7] = 0
    with pytest.raises(AssertionError, match='masks: 1 store.s. AFTER the operand, nearest 1 element'):
        mc()


def test_an_empty_operand_is_two_bands():
    ev, ec = guarded((0, 4), torch.float64, 'cpu', name='box2d_out')
    assert ev.shape == (0, 4) and ec.buf.numel() == 2 * G
    ec(written=True)
    ec.buf[G] = 1.0
    with pytest.raises(AssertionError, match='box2d_out: 1 store.s. AFTER the operand, nearest 1 element'):
        ec()


def test_scale_table_holds_exactly_roundup4_floats():
    """the t3d.h contract for scale / shift: roundup4(K) floats, NaN right behind"""
    K = 6
    t = torch.ones(roundup4(K))
    sv, sc = guarded((roundup4(K),), torch.float32, 'cpu', fill=t, name='scale')
    assert sv.numel() == 8 and torch.isnan(sc.buf[G + 8]) and torch.isnan(sc.buf[G - 1])
