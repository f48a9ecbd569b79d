"""The dense 3x3 convolution epos_conv3x3_f32 -- an implicit GEMM inside the CONV instantiations
of pointwise_gemm_h2_f32 (csrc/pointwise_gemm_h2.hip) and pointwise_gemm_split_f32 (csrc/
pointwise_gemm_split.hip) -- in every launch regime of tests/helpers/conv3x3_cases.py, through
the C ABI of the product library and through both kernels. Every case asserts
 (a) exactness: on integer data the output equals the fp64 reference cast to float32 bit for bit
     (-0.0 read as 0.0), whatever the slot says;
 (b) accuracy on normal and relu-like data: |got - ref| <= H2_MAX_REL_ERR * mag elementwise, mag =
     sum |x||w| + |bias|, finite output; a stale slot widens the bar by its scale ratio; K = 4608
     (cin512) is held to the larger of that bar and 1.5 x the error of a float32 numpy product;
 (c) no stray access: Y lies in a sentinel-filled buffer with guard rows in front and behind, X
     between NaN rows with NaN in its padding columns -- also where the library measures X itself;
 (d) the same bytes in two consecutive runs, with the h2 narrow-tile limit at 0 and at 2^30, with
     a measured and a given exact slot; and below: after another launch, on a side stream, in a
     captured graph, image by image;
 (e) y_amax == max |Y| exactly.
The inputs and fp64 expectations are computed once per case and kind (the helpers' lru_cache).

Measured on an MI355X, worst |got - ref| / mag (RECORDED, not asserted; the bar is 4e-7): over the
table 1.72e-7 for h2 (s1_measured, relu_like) and 1.42e-7 for split (rows128, relu_like); at
K = 4608 (cin512) 4.16e-8 for h2 and 4.58e-8 for split against 3.55e-8 for the float32 numpy
product. Every 'int' case is bit-equal in both kernels."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import conv3x3_cases as cc

pytestmark = pytest.mark.gpu

CASES = cc.by_name(cc.CASES)
SENT = np.int32(cc.SENTINEL_BITS)
ITEMS = [(c.name, k) for c in cc.CASES for k in cc.KERNELS]


@pytest.fixture(scope='module')
def lib():
  from epos_amd import _lib
  assert torch.cuda.is_available(), 'GPU tests need a HIP device'
  return _lib.load()


@pytest.fixture(autouse=True)
def tile_limit(lib):
  """The tests set epos_set_h2_narrow_tile_limit; the process's value comes back."""
  prev = lib.epos_set_h2_narrow_tile_limit(0)
  lib.epos_set_h2_narrow_tile_limit(prev)
  yield
  lib.epos_set_h2_narrow_tile_limit(prev)


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(words):
  """A uint32 / int32 / float32 host array on the device, bit for bit, as int32."""
  return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).cuda()


def _sentinels(*shape):
  return torch.full(shape, cc.SENTINEL_BITS, dtype=torch.int32, device='cuda')


def _pack(lib, w, which):
  k, n = w.shape
  fn = {'plain': lib.epos_pack_pointwise_weights, 'h2': lib.epos_pack_pointwise_weights_h2,
        'split': lib.epos_pack_pointwise_weights_split}[which]
  w = np.ascontiguousarray(w, np.float32)
  src = w.ctypes.data_as(ctypes.c_void_p)
  total = fn(src, k, n, None)
  assert total > 0, which
  dst = np.empty(total, np.float32 if which == 'plain' else np.uint8)
  fn(src, k, n, dst.ctypes.data_as(ctypes.c_void_p))
  return torch.from_numpy(dst).cuda()


def _bits(x):
  return int(np.float32(x).view(np.uint32))


def _slot(word=None, at=0):
  from epos_amd import _lib
  s = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device='cuda')
  if word is not None:
    s[at] = int(np.array([word], np.uint32).view(np.int32)[0])
  return s


def _slot_value(slot):
  return float(slot.cpu().numpy().view(np.float32).max())


def _bias_dev(bias, n):
  """round_up(N, 128) floats, NaN behind the N values."""
  b = np.full(-(-n // 128) * 128, np.nan, np.float32)
  b[:n] = bias
  return _dev(b)


class Conv(object):
  """One case's inputs of one value kind on the device, its launches and their outputs."""

  def __init__(self, lib, case, kind):
    self.lib, self.case, self.kind = lib, case, kind
    inp = cc.inputs(case.name, kind)
    self.X = _dev(cc.x_buffer(case, kind))
    assert self.X.data_ptr() % 16 == 0
    self.x_ptr = self.X.data_ptr() + 4 * cc.x_guard_rows(case) * case.ldx
    wkn = inp.w.reshape(9 * case.cin, case.cout)
    self.Wp, self.Wh, self.Ws = (_pack(lib, wkn, k) for k in ('plain', 'h2', 'split'))
    self.bias = _bias_dev(inp.bias, case.cout) if case.bias else None
    word = cc.slot_word(case, inp.true_max)
    self.slot = _slot(word, 37) if word is not None else None      # None: x_amax == NULL
    self.exact_slot = _slot(_bits(inp.true_max), 11)

  def buffers(self, m=None):
    """Fresh outputs: (the Y buffer, the y_amax slot or None)."""
    y = _sentinels(cc.y_layout(self.case, m).floats)
    assert y.data_ptr() % 512 == 0
    return y, (_slot(0x7fc00000, 3) if self.case.y_amax else None)     # cleared by the launch

  def args(self, out, kernel, slot='case', image=None):
    """kernel 'h2': Wh and Ws both come along and Wh wins; 'split': Ws alone. image: that image
    alone, into a buffer of its own."""
    from epos_amd import _lib
    c = self.case
    ybuf, yslot = out
    slot = self.slot if isinstance(slot, str) else slot
    h2 = kernel == 'h2'
    x = self.x_ptr + (0 if image is None else 4 * image * c.h * c.w * c.ldx)
    m = None if image is None else cc.m_of(c) // c.b
    return _lib.Conv3x3Args(
        X=x, ldx=c.ldx, Wp=self.Wp.data_ptr(),
        bias=self.bias.data_ptr() if self.bias is not None else None,
        Y=ybuf.data_ptr() + 4 * cc.y_layout(c, m).off, ldy=c.ldy,
        B=c.b if image is None else 1, H=c.h, W=c.w, Cin=c.cin, Cout=c.cout, stride=c.stride,
        rate=c.rate, relu=c.relu, Ws=self.Ws.data_ptr(), Wh=self.Wh.data_ptr() if h2 else None,
        x_amax=slot.data_ptr() if h2 and slot is not None else None,
        y_amax=yslot.data_ptr() if yslot is not None else None)

  def launch(self, out, kernel, limit=0, **kw):
    """Enqueues the conv on the current stream."""
    from epos_amd import _lib
    self.lib.epos_set_h2_narrow_tile_limit(limit)
    a = self.args(out, kernel, **kw)
    if out[1] is not None:
      _lib.check(self.lib.epos_amax_clear(out[1].data_ptr(), 1, _stream()), 'amax_clear')
    _lib.check(self.lib.epos_conv3x3_f32(ctypes.byref(a), _stream()),
               '%s %s' % (self.case.name, kernel))

  @staticmethod
  def fetch(out):
    return out[0].cpu().numpy(), (_slot_value(out[1]) if out[1] is not None else None)

  def run(self, kernel, m=None, **kw):
    out = self.buffers(m)
    self.launch(out, kernel, **kw)
    torch.cuda.synchronize()
    return self.fetch(out)

  def values(self, ybuf, m=None):
    return ybuf[cc.y_index(self.case, m)].view(np.float32)


def _same(a, b, what):
  diff = np.flatnonzero(a[0] != b[0])
  assert diff.size == 0, '%s: %d words of Y differ (first at %d)' % (what, diff.size, diff[0])
  assert a[1] == b[1], (what, a[1], b[1])


def _check_writes(case, ybuf, m=None):
  """(c): everything the case must write is written, every other word keeps the sentinel."""
  mask = cc.written_mask(case, m)
  left = int((ybuf[mask] == SENT).sum())
  assert left == 0, '%s: %d elements unwritten' % (case.name, left)
  broken = np.flatnonzero(ybuf[~mask] != SENT)
  assert broken.size == 0, '%s: %d words written outside [M) x [y_off, y_off + Cout) (first at ' \
      'index %d of the outside)' % (case.name, broken.size, broken[0])


def _check_exact(g, got, kernel):
  """(a)"""
  ref, _ = cc.expected(g.case.name, 'int')
  want = ref.astype(np.float32)
  bad = np.argwhere((got + np.float32(0)).view(np.uint32) != want.view(np.uint32))
  assert bad.size == 0, '%s %s: %d of %d elements differ from the exact result, first at row ' \
      '%d column %d: got %r, exact %r' % (g.case.name, kernel, len(bad), got.size, bad[0][0],
                                          bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


def _bar(case, kind):
  """The bound of (b) relative to mag, and the error of the float32 product it may rest on."""
  bar = cc.H2_MAX_REL_ERR
  e32 = None
  if case.name == 'cin512':
    e32 = cc.fp32_product_error(case.name, kind)
    bar = max(bar, 1.5 * e32)
  return bar, e32


def _check_accuracy(g, got, kernel):
  """(b); returns the worst |got - ref| / mag."""
  case = g.case
  ref, mag = cc.expected(case.name, g.kind)
  assert np.isfinite(got).all(), '%s %s: non-finite output' % (case.name, kernel)
  assert (mag > 0).all()
  bar, e32 = _bar(case, g.kind)
  if kernel == 'h2':
    bar *= cc.scale_ratio(case, cc.inputs(case.name, g.kind).true_max)
  rel = np.abs(got.astype(np.float64) - ref) / mag
  worst = float(rel.max())
  print('%s %s %s (M %d, N %d, K %d): worst |got - ref| / mag = %.3e, bar %.3e%s' % (
      case.name, kernel, g.kind, cc.m_of(case), case.cout, 9 * case.cin, worst, bar,
      '' if e32 is None else ', float32 numpy product %.3e' % e32))
  assert worst <= bar, (case.name, kernel, g.kind, worst, bar)
  return worst


def _check_amax(g, res):
  """(e)"""
  if g.case.y_amax:
    top = float(np.abs(g.values(res[0])).max())
    assert res[1] == top and top > 0, (g.case.name, res[1], top)
  else:
    assert res[1] is None


@pytest.mark.parametrize('name,kernel', ITEMS)
def test_conv3x3_regime(lib, name, kernel):
  case = CASES[name]
  assert cc.kernel_taken(kernel == 'h2', True, cc.m_of(case)) == kernel
  for kind in case.kinds:
    g = Conv(lib, case, kind)
    res = g.run(kernel)
    _check_writes(case, res[0])
    got = g.values(res[0])
    if kind == 'int':
      _check_exact(g, got, kernel)
    else:
      _check_accuracy(g, got, kernel)
    _check_amax(g, res)
    # (d) two consecutive runs; a conv never takes the narrow tile; measured == given exact slot
    what = '%s %s %s' % (name, kernel, kind)
    _same(res, g.run(kernel), what + ': second run')
    if kernel == 'h2':
      _same(res, g.run(kernel, limit=cc.BIG), what + ': narrow-tile limit 2^30')
      if case.slot == 'measured':
        _same(res, g.run(kernel, slot=g.exact_slot), what + ': given exact slot')


@pytest.mark.parametrize('kernel', cc.KERNELS)
def test_conv3x3_y_amax_sees_every_row_and_column_block(lib, kernel):
  """The maximum of |Y| planted in turn into the first row, the last valid row of the ragged last
  row tile, and column 0 and column Cout - 1 of the second column tile (one pixel of X large, the
  others a hundredth of it, w >= 0 with the weight on the centre tap, one large bias): the slot
  holds exactly that element every time."""
  from epos_amd import _lib
  b, h, w, cin, cout = 1, 11, 13, 32, 200
  m = b * h * w
  assert m % 128 and m > 128 and 128 < cout <= 256
  rng = np.random.default_rng(5)
  base = np.maximum(rng.standard_normal((m, cin)), 0).astype(np.float32) * np.float32(0.01)
  wgt = np.abs(rng.standard_normal((3, 3, cin, cout)) / np.sqrt(cin)).astype(np.float32)
  wgt *= np.float32(0.05)
  wgt[1, 1] *= np.float32(20)
  wkn = wgt.reshape(9 * cin, cout)
  Wp, Wh, Ws = (_pack(lib, wkn, k) for k in ('plain', 'h2', 'split'))
  slot = _slot(_bits(4.0), 11)
  for r, c in ((0, 5), (m - 1, 40), (70, 128), (m - 1, 128), (0, cout - 1), (m - 1, cout - 1),
               (127, 127), (128, 0)):
    x = base.copy()
    x[r] = rng.uniform(2, 4, cin).astype(np.float32)
    bias = np.zeros(cout, np.float32)
    bias[c] = 50
    X, Bd = _dev(x), _bias_dev(bias, cout)
    Y, ys = _sentinels(m, cout), _slot(0x7fc00000, 9)
    args = _lib.Conv3x3Args(X=X.data_ptr(), ldx=cin, Wp=Wp.data_ptr(), bias=Bd.data_ptr(),
                            Y=Y.data_ptr(), ldy=cout, B=b, H=h, W=w, Cin=cin, Cout=cout, stride=1,
                            rate=1, relu=0, Ws=Ws.data_ptr(),
                            Wh=Wh.data_ptr() if kernel == 'h2' else None,
                            x_amax=slot.data_ptr() if kernel == 'h2' else None,
                            y_amax=ys.data_ptr())
    _lib.check(lib.epos_amax_clear(ys.data_ptr(), 1, _stream()))
    _lib.check(lib.epos_conv3x3_f32(ctypes.byref(args), _stream()))
    torch.cuda.synchronize()
    got = Y.cpu().numpy().view(np.float32)
    assert np.isfinite(got).all()
    assert np.unravel_index(np.abs(got).argmax(), got.shape) == (r, c)
    assert _slot_value(ys) == float(np.abs(got).max()), (r, c)


# ----------------------------------------------------------------------------- refusals ---
@pytest.mark.parametrize('what', cc.REFUSALS)
def test_conv3x3_refusals(lib, what):
  """Each of these is refused by the entry point before anything is launched: the return value
  is an error with a message, Y keeps its sentinels, the y_amax slot its content, and the same
  arguments without the fault give the exact result."""
  case = CASES[cc.REFUSAL_CASE]
  g = Conv(lib, case, 'int')
  out = g.buffers()
  a = g.args(out, 'h2')
  if what == 'null_x':
    a.X = None
  elif what == 'null_wp':
    a.Wp = None
  elif what == 'null_y':
    a.Y = None
  elif what == 'cin_48':
    a.Cin = 48
  elif what == 'ldx_lt_cin':
    a.ldx = case.cin - 4
  elif what == 'ldx_mod_4':
    a.ldx = case.cin + 2
  elif what == 'x_unaligned':
    a.X = g.x_ptr + 4
  elif what == 'stride_3':
    a.stride = 3
  elif what == 'rate_0':
    a.rate = 0
  elif what == 'b_0':
    a.B = 0
  elif what == 'no_wh_no_ws':           # the product library carries no fp32-MFMA kernel
    a.Wh = a.Ws = None
  elif what == 'm_8':                   # B*Ho*Wo <= 8: neither product kernel takes it
    a.B, a.H, a.W, a.y_amax = 1, 2, 4, None
  elif what == 'y_amax_cout_mod_4':
    a.Cout = case.cout - 1
  elif what == 'y_amax_ldy_mod_4':
    a.ldy = case.ldy + 1
  else:
    assert what == 'y_amax_y_unaligned'
    a.Y = a.Y + 4
  for limit in (0, cc.BIG):
    lib.epos_set_h2_narrow_tile_limit(limit)
    rc = lib.epos_conv3x3_f32(ctypes.byref(a), _stream())
    assert rc != 0 and lib.epos_last_error(), what
  torch.cuda.synchronize()
  assert bool((out[0] == cc.SENTINEL_BITS).all()), what
  assert out[1].cpu().numpy().view(np.uint32).max() == 0x7fc00000, what
  # ... and the same arguments without the fault run
  res = g.run('h2')
  _check_writes(case, res[0])
  _check_exact(g, g.values(res[0]), 'h2')
  _check_amax(g, res)


# ---------------------------------------------------- history, stream, graph, image-wise ---
@pytest.mark.parametrize('kernel', cc.KERNELS)
def test_conv3x3_launch_is_independent_of_the_one_before(lib, kernel):
  """X, then a different case Y (other Cin, rate, tile count and K-step count), then X again,
  back to back on the stream: each gives the bytes it gives alone."""
  gx, gy = (Conv(lib, CASES[n], 'int') for n in cc.HISTORY_PAIR)
  x0, y0 = gx.run(kernel), gy.run(kernel)
  _check_writes(gx.case, x0[0])
  _check_writes(gy.case, y0[0])
  _check_exact(gx, gx.values(x0[0]), kernel)
  _check_exact(gy, gy.values(y0[0]), kernel)
  ox, oy, ox2 = gx.buffers(), gy.buffers(), gx.buffers()
  gx.launch(ox, kernel)
  gy.launch(oy, kernel)
  gx.launch(ox2, kernel)
  torch.cuda.synchronize()
  _same(x0, Conv.fetch(ox), 'X before Y')
  _same(y0, Conv.fetch(oy), 'Y after X')
  _same(x0, Conv.fetch(ox2), 'X after Y')


@pytest.mark.parametrize('kernel', cc.KERNELS)
def test_conv3x3_on_a_non_default_stream(lib, kernel):
  case = CASES[cc.STREAM_CASE]
  g = Conv(lib, case, case.kinds[-1])
  ref = g.run(kernel)
  _check_writes(case, ref[0])
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  with torch.cuda.stream(s):
    assert torch.cuda.current_stream().cuda_stream == s.cuda_stream
    out = g.run(kernel)
  _same(ref, out, 'non-default stream')


@pytest.mark.parametrize('kernel', cc.KERNELS)
def test_conv3x3_in_a_captured_graph(lib, kernel):
  """One launch (with its epos_amax_clear) captured on a single stream, after an eager one (the
  first fp16-pair launch on a device allocates), and replayed twice into re-sentinelled
  buffers: the eager bytes."""
  case = CASES[cc.GRAPH_CASE]
  g = Conv(lib, case, 'int')
  eager = g.run(kernel)
  _check_writes(case, eager[0])
  _check_exact(g, g.values(eager[0]), kernel)
  out = g.buffers()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    g.launch(out, kernel)
  for _ in range(2):
    out[0].fill_(cc.SENTINEL_BITS)
    graph.replay()
    torch.cuda.synchronize()
    _same(eager, Conv.fetch(out), 'graph replay')


@pytest.mark.parametrize('kernel', cc.KERNELS)
def test_conv3x3_image_by_image(lib, kernel):
  """Each image of the B = 3 case launched alone (same slot) gives its rows of the batch launch:
  nothing of an image depends on its neighbours in the batch, though they share a row tile."""
  case = CASES[cc.IMAGES_CASE]
  hw = cc.m_of(case) // case.b
  for kind in case.kinds:
    g = Conv(lib, case, kind)
    batch = g.values(g.run(kernel)[0])
    for i in range(case.b):
      one = g.run(kernel, m=hw, image=i)
      _check_writes(case, one[0], hw)
      got = g.values(one[0], hw)
      assert np.array_equal(got.view(np.uint32), batch[i * hw:(i + 1) * hw].view(np.uint32)), \
          '%s %s: image %d alone differs from the batch' % (kernel, kind, i)
      assert one[1] == float(np.abs(got).max())
