"""Guard bands around the operands of a kernel launch (a plain helper, no fixtures).

A kernel test whose tensors are exactly the operand's size cannot see what the kernel touches outside them: a load past the last
column, the last row or the end of a per-channel table reads a neighbouring allocation, and the products that use those values are
usually masked or never stored; a stray store lands in allocator slack.  `guarded` therefore puts every operand into the middle of
ONE flat allocation of its own:

  input   the valid elements hold the caller's values; the front band, the back band and, with a leading dimension `ld` wider than
          the valid columns, every row's padding hold NaN (integer operands: the type's minimum, an index no kernel accepts).  A result that
          used one of them is NaN (or wildly out of range) where the fp64 reference is finite: `assert_clean`.  The checker asserts
          that the launch changed nothing in the whole allocation.
  output  the interior, the row padding and both bands are pre-filled with one sentinel bit pattern (a NaN with a payload no
          arithmetic produces).  The checker asserts that bands and padding still hold it bit for bit and, with `written=True`,
          that no interior element does.

Every band is `G` = 256 elements, so an overrun of up to 256 elements in either direction stays inside an allocation the test owns:
a wrong kernel reads NaN, never foreign memory.  Failures name the operand.
"""
import torch

G = 256
INT_BAND = -2 ** 31
INT64_BAND = -2 ** 63
SENTINEL = object()          # fill=SENTINEL: an output operand

# quiet NaNs with a payload (a kernel that produces a NaN produces the canonical one, 0x7FC00000 / 0x7FC0 / 0x7FF8000000000000), and
# an unlikely index.  torch.int64 also stands for a uint64 operand (a scratch of bit masks): the caller passes its address as uint64.
_SENT_BITS = {torch.float32: (torch.int32, 0xFFC5A3E1 - (1 << 32)), torch.bfloat16: (torch.int16, 0xFFD5 - (1 << 16)),
              torch.float64: (torch.int64, 0xFFF8C5A3E1B2D497 - (1 << 64)), torch.int32: (torch.int32, -0x7FFFFFFF),
              torch.int64: (torch.int64, -0x7FFFFFFFC5A3E1B3)}
_IN_FILL = {torch.int32: INT_BAND, torch.int64: INT64_BAND}          # every other type: NaN


def roundup4(k):
    return (k + 3) // 4 * 4


def _bits(t):
    return t.view(_SENT_BITS[t.dtype][0])


class Check:
    """What `guarded` returns next to the view.  check() / check(written=True) after the launch (written=None: an output that the
    launch must leave untouched, interior included); `.valid` is the view of the valid elements ([rows, width] at column `col0` of the
    [rows, ld] interior), `.buf` the whole flat allocation, `.ptr` the interior's address (the view's data_ptr(), also for an operand
    of no elements, whose view has none)."""

    def __init__(self, name, buf, view, valid, front, n_int, is_out, pad_mask):
        self.name, self.buf, self.view, self.valid = name, buf, view, valid
        self._front, self._n, self._out, self._pad = front, n_int, is_out, pad_mask
        self._before = None if is_out else buf.clone()
        self.ptr = buf.data_ptr() + front * buf.element_size()

    def __call__(self, written=False):
        name, b = self.name, _bits(self.buf)
        if not self._out:
            same = torch.equal(b, _bits(self._before))
            assert same, '%s: the launch changed an INPUT operand (or its bands) at flat offsets %s' % (
                name, (b != _bits(self._before)).nonzero().flatten()[:8].tolist())
            return
        sent = _SENT_BITS[self.buf.dtype][1]
        front, back = b[:self._front], b[self._front + self._n:]
        bad = (front != sent).nonzero().flatten()
        assert bad.numel() == 0, '%s: %d store(s) BEFORE the operand, nearest %d element(s) ahead of it' % (
            name, bad.numel(), self._front - int(bad.max()))
        bad = (back != sent).nonzero().flatten()
        assert bad.numel() == 0, '%s: %d store(s) AFTER the operand, nearest %d element(s) past its end' % (
            name, bad.numel(), int(bad.min()) + 1)
        inner = b[self._front:self._front + self._n]
        if self._pad is not None:
            bad = ((inner != sent) & self._pad).nonzero().flatten()
            assert bad.numel() == 0, '%s: %d store(s) into the row PADDING (interior offsets %s)' % (name, bad.numel(), bad[:8].tolist())
        if written is None:
            assert bool((inner == sent).all()), '%s: %d element(s) written by a launch that must not touch it (first interior offsets %s)' % (
                name, int((inner != sent).sum()), (inner != sent).nonzero().flatten()[:8].tolist())
        if written:
            un = inner == sent
            if self._pad is not None:
                un = un & ~self._pad
            assert not bool(un.any()), '%s: %d element(s) never written (first interior offsets %s)' % (
                name, int(un.sum()), un.nonzero().flatten()[:8].tolist())


def guarded(shape, dtype, device, ld=None, front=G, back=G, fill=SENTINEL, col0=0, name='operand'):
    """One flat allocation [front band | interior | back band]; returns (view, check).

    shape   the valid elements, any rank; with `ld` / `col0` it is read as [rows, width]
    ld      leading dimension of the interior in elements (default: the width, a dense operand); the valid columns are
            col0 .. col0 + width - 1 of each row of `ld`
    fill    SENTINEL (default): an output operand.  A tensor of `shape` (any device; converted to `dtype`): an input operand
    view    the tensor whose data_ptr() is the ABI pointer: `shape` itself for a dense operand, else the [rows, ld] interior"""
    shape = tuple(int(s) for s in shape)
    assert dtype in _SENT_BITS, dtype
    assert front >= G and back >= G, 'bands of at least %d elements' % G
    strided = ld is not None or col0
    if strided:
        rows, width = (shape if len(shape) == 2 else (1, shape[0]))
        ld = width if ld is None else int(ld)
        assert col0 >= 0 and col0 + width <= ld, (col0, width, ld)
        n = rows * ld
    else:
        n = 1
        for s in shape:
            n *= s
    is_out = fill is SENTINEL
    buf = torch.empty(front + n + back, dtype=dtype, device=device)
    if is_out:
        _bits(buf).fill_(_SENT_BITS[dtype][1])
    else:
        buf.fill_(_IN_FILL.get(dtype, float('nan')))
    inner = buf[front:front + n]
    pad = None
    if strided:
        view = inner.view(rows, ld)
        valid = view[:, col0:col0 + width]
        if ld != width:
            pad = torch.ones(rows, ld, dtype=torch.bool, device=device)
            pad[:, col0:col0 + width] = False
            pad = pad.flatten()
    else:
        view = valid = inner.view(shape)
    if not is_out:
        valid.copy_(torch.as_tensor(fill).to(device=device, dtype=dtype).reshape(valid.shape))
    return view, Check(name, buf, view, valid, front, n, is_out, pad)


def assert_clean(name, got, ref):
    """The detection rule for inputs: a NaN (or inf) anywhere in an output that the fp64 reference says is finite means that the
    kernel consumed a band or padding value."""
    got, ref = got.double(), torch.as_tensor(ref).double().to(got.device)
    bad = ~torch.isfinite(got) & torch.isfinite(ref)
    assert not bool(bad.any()), '%s: %d non-finite element(s) where the reference is finite -- a band / padding value was consumed ' \
                                '(first flat offsets %s)' % (name, int(bad.sum()), bad.flatten().nonzero().flatten()[:8].tolist())
