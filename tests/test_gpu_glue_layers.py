"""The glue-layer kernels (csrc/glue.hip, csrc/layers.hip, csrc/softmax.hip, the bf16 mean in
csrc/bf16.hip) over the shape tables of tests/helpers/glue_cases.py, each through its C entry point: inputs sit
at their pitch and base offset inside a larger allocation whose padding holds NaN; the output
allocation starts as a sentinel bit pattern (a NaN payload for fp32, SENT for bf16, -1 for integers) in its padding
columns, before the base and in a guard region behind the last row, and all of that must survive.
Exact operations must be array_equal to numpy; resize (fp32) and the three means must give the
bits of the float32 restatements of tests/helpers/glue_ref.py (which tests/test_glue_cases_host.py
holds to derived bounds against float64). Every case runs twice into fresh buffers and must give
the same bits."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import glue_cases as gc
from helpers import glue_ref as gr
from helpers.bf16_ref import bf16_round_bits, bf16_to_f32

pytestmark = pytest.mark.gpu

SENT32 = 0x7fa5a5a5        # a NaN bit pattern no computed value has
SENT = 0x7FC1              # the bf16 tests' NaN pattern
GUARD = 64                 # elements behind the last row
E_INVALID = -1


def _lib():
  from epos_amd import _lib as L
  return L, L.load()


def _p(t, off=0):
  return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _names(table):
  return [c.name for c in table]


class In(object):
  """x [..., c] at pitch ld and element offset off inside a NaN-filled allocation."""

  def __init__(self, x, ld, off=0, bf16=False):
    c = x.shape[-1]
    rows = x.size // c
    if bf16:
      bits = bf16_round_bits(x).reshape(rows, c)
      assert np.array_equal(bf16_to_f32(bits).reshape(x.shape), x), 'input not bf16 values'
      self.buf = torch.full((off + rows * ld,), SENT, dtype=torch.int16, device='cuda')
      src = torch.from_numpy(bits.view(np.int16).copy())
    else:
      self.buf = torch.full((off + rows * ld,), float('nan'), device='cuda')
      src = torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(rows, c))
    self.buf[off:].view(rows, ld)[:, :c] = src.cuda()
    self.ptr = _p(self.buf, off)
    assert self.buf.data_ptr() % 256 == 0


class Out(object):
  """rows x c payload at pitch ld and offset off inside a sentinel-filled allocation."""
  KINDS = {'f32': (torch.int32, SENT32), 'bf16': (torch.int16, SENT), 'i64': (torch.int64, -1)}

  def __init__(self, rows, c, ld, off=0, kind='f32'):
    dtype, self.sent = self.KINDS[kind]
    self.rows, self.c, self.ld, self.off = rows, c, ld, off
    self.buf = torch.full((off + rows * ld + GUARD,), self.sent, dtype=dtype, device='cuda')
    self.ptr = _p(self.buf, off)
    assert self.buf.data_ptr() % 256 == 0

  def read(self):
    """The payload's raw bits [rows, c]; asserts that every sentinel element is unchanged."""
    torch.cuda.synchronize()
    raw = self.buf.cpu().numpy()
    n = self.rows * self.ld
    assert (raw[:self.off] == self.sent).all(), 'write before the base'
    assert (raw[self.off + n:] == self.sent).all(), 'write behind the last row'
    body = raw[self.off:self.off + n].reshape(self.rows, self.ld)
    assert (body[:, self.c:] == self.sent).all(), 'write into the padding columns'
    return np.ascontiguousarray(body[:, :self.c])


def _twice(run):
  """run() -> raw payload bits; two runs into fresh buffers must agree bit for bit."""
  a, b = run(), run()
  assert np.array_equal(a, b), 'two runs differ'
  return a


def _f32(raw):
  return raw.view(np.float32)


def _bits32(x):
  return np.ascontiguousarray(x, np.float32).view(np.int32)


def _half_ulp(x):
  """half a bf16 ulp of |x| (0 at 0): 2^(floor(log2|x|) - 8)"""
  x = np.abs(x)
  return np.where(x > 0, np.ldexp(1.0, np.frexp(x)[1] - 9), 0.0)


# --------------------------------------------------------------------------------- means ---
@pytest.mark.parametrize('name', _names(gc.MEAN))
def test_global_avg_pool_f32(name):
  L, lib = _lib()
  c = gc.by_name(gc.MEAN)[name]
  x = gr.mean_input(c)

  def run():
    X, Y = In(x, c.ldx, c.off), Out(c.b, c.c, c.c, 4)
    L.check(lib.epos_global_avg_pool_f32(X.ptr, c.ldx, Y.ptr, c.b, c.hw, c.c, _stream()), name)
    return Y.read()
  got = _twice(run)
  want = gr.mean_f32(x, 64)
  print(name, 'max |got - f64| =', np.abs(_f32(got) - gr.mean_f64(x)).max())
  assert np.array_equal(got, _bits32(want))


@pytest.mark.parametrize('name', _names(gc.PARTIAL))
def test_global_avg_pool_partial_f32(name):
  L, lib = _lib()
  c = gc.by_name(gc.PARTIAL)[name]
  x = gr.partial_input(c)

  def run():
    X, Y = In(x, c.ldp, c.off), Out(c.b, c.c, c.c, 4)
    L.check(lib.epos_global_avg_pool_partial_f32(X.ptr, c.ldp, Y.ptr, c.b, c.blocks, c.c, c.hw,
                                                 _stream()), name)
    return Y.read()
  assert np.array_equal(_twice(run), _bits32(gr.mean_f32(x, 16, c.hw)))


@pytest.mark.parametrize('name', _names(gc.MEAN_BF16))
def test_global_avg_pool_bf16(name):
  L, lib = _lib()
  c = gc.by_name(gc.MEAN_BF16)[name]
  x = gr.mean_input(c, bf16=True)

  def run():
    X, Y = In(x, c.ldx, c.off, bf16=True), Out(c.b, c.c, c.c, 4)
    L.check(lib.epos_global_avg_pool_bf16(X.ptr, c.ldx, Y.ptr, c.b, c.hw, c.c, _stream()), name)
    return Y.read()
  assert np.array_equal(_twice(run), _bits32(gr.mean_f32(x, 32)))


# -------------------------------------------------------------------------------- resize ---
@pytest.mark.parametrize('name', _names(gc.RESIZE))
def test_resize_bilinear_f32(name):
  L, lib = _lib()
  c = gc.by_name(gc.RESIZE)[name]
  x = gr.resize_input(c)

  def run():
    X, Y = In(x, c.ldx, c.xoff), Out(c.b * c.ho * c.wo, c.c, c.ldy, c.yoff)
    L.check(lib.epos_resize_bilinear_f32(X.ptr, c.ldx, Y.ptr, c.ldy, c.b, c.hi, c.wi, c.ho, c.wo,
                                         c.c, _stream()), name)
    return Y.read()
  got = _twice(run).reshape(c.b, c.ho, c.wo, c.c)
  want, _ = gr.resize_f32(x, c.ho, c.wo)
  assert np.array_equal(got, _bits32(want))
  if (c.hi, c.wi) == (1, 1):                               # the broadcast is a copy
    assert np.array_equal(_f32(got), np.broadcast_to(x, got.shape))


RESIZE_BF16_IDS = [(c.name, 0) for c in gc.RESIZE_BF16] + \
    [(c.name, 1) for c in gc.RESIZE_BF16 if c.hi * c.wi <= 300]


@pytest.mark.parametrize('name,src_f32', RESIZE_BF16_IDS,
                         ids=['%s-%s' % (n, 'f32src' if s else 'bf16src')
                              for n, s in RESIZE_BF16_IDS])
def test_resize_bilinear_bf16(name, src_f32):
  """The fp32 kernel's arithmetic in numpy's float32, then one RNE: half a bf16 ulp, plus a few
  fp32 roundings of the corner values where the interpolation cancels (the bound of
  tests/test_gpu_bf16_kernels.py)."""
  L, lib = _lib()
  c = gc.by_name(gc.RESIZE_BF16)[name]
  x = gr.resize_input(c, bf16=not src_f32)

  def run():
    X = In(x, c.ldx, c.xoff, bf16=not src_f32)
    Y = Out(c.b * c.ho * c.wo, c.c, c.ldy, c.yoff, 'bf16')
    L.check(lib.epos_resize_bilinear_bf16(X.ptr, c.ldx, int(src_f32), Y.ptr, c.ldy, c.b, c.hi,
                                          c.wi, c.ho, c.wo, c.c, _stream()), name)
    return Y.read()
  raw = _twice(run).view(np.uint16).reshape(c.b, c.ho, c.wo, c.c)
  got = bf16_to_f32(raw).astype(np.float64)
  want, (tl, tr, bl, br) = gr.resize_f32(x, c.ho, c.wo)
  mag = np.abs(tl) + np.abs(tr) + np.abs(bl) + np.abs(br)
  assert (np.abs(got - want) <= _half_ulp(want) + 2.0 ** -21 * mag).all()


@pytest.mark.parametrize('name', _names(gc.RESIZE))
def test_resize_entry_points_agree(name):
  """Device against device: the three entry points that resize share one sampler (csrc/nhwc.h)
  and must not drift apart. epos_resize_merge_f32 with one source gives the bits of
  epos_resize_bilinear_f32; epos_resize_bilinear_bf16 gives the round-to-nearest-even bf16 of
  the fp32 entry's output on the same input, from an fp32 source (x_f32 = 1) and from a bf16
  source (x_f32 = 0, on an input that holds bf16 values). Out.read() holds the padding."""
  L, lib = _lib()
  c = gc.by_name(gc.RESIZE)[name]
  rows = c.b * c.ho * c.wo

  def f32_entry(x):
    X, Y = In(x, c.ldx, c.xoff), Out(rows, c.c, c.ldy, c.yoff)
    L.check(lib.epos_resize_bilinear_f32(X.ptr, c.ldx, Y.ptr, c.ldy, c.b, c.hi, c.wi, c.ho, c.wo,
                                         c.c, _stream()), name)
    return Y.read()

  def bf16_entry(x, src_f32):
    X, Y = In(x, c.ldx, c.xoff, bf16=not src_f32), Out(rows, c.c, c.ldy, c.yoff, 'bf16')
    L.check(lib.epos_resize_bilinear_bf16(X.ptr, c.ldx, int(src_f32), Y.ptr, c.ldy, c.b, c.hi,
                                          c.wi, c.ho, c.wo, c.c, _stream()), name)
    return Y.read().view(np.uint16)

  x = gr.resize_input(c)
  want = f32_entry(x)
  X, Y = In(x, c.ldx, c.xoff), Out(rows, c.c, c.ldy, c.yoff)
  src = (L.ResizeSrc * 1)(L.ResizeSrc(X.ptr, c.ldx, c.hi, c.wi))
  L.check(lib.epos_resize_merge_f32(src, 1, Y.ptr, c.ldy, c.b, c.ho, c.wo, c.c, L.MERGE_MAX,
                                    _stream()), name)
  assert np.array_equal(Y.read(), want)
  if not gc.bf16_ok(c):
    return
  assert np.array_equal(bf16_entry(x, True), bf16_round_bits(_f32(want)))
  xb = gr.resize_input(c, bf16=True)
  assert np.array_equal(bf16_entry(xb, False), bf16_round_bits(_f32(f32_entry(xb))))


# ------------------------------------------------------------------- max pool, subsample ---
def _nhwc_case(table, name, bf16, make_x, ref, launch, out_hw):
  c = gc.by_name(table)[name]
  x = make_x(c, bf16=bf16)
  ho, wo = out_hw(c)

  def run():
    X = In(x, c.ldx, c.xoff, bf16=bf16)
    Y = Out(c.b * ho * wo, c.c, c.ldy, c.yoff, 'bf16' if bf16 else 'f32')
    launch(c, X, Y)
    return Y.read()
  raw = _twice(run)
  want = ref(c, x)
  assert want.shape == (c.b, ho, wo, c.c)
  got = bf16_to_f32(raw.view(np.uint16)) if bf16 else _f32(raw)
  assert np.array_equal(got.reshape(want.shape), want)
  wbits = bf16_round_bits(want).view(np.int16) if bf16 else _bits32(want)
  assert np.array_equal(raw.reshape(want.shape), wbits)


def _pool_hw(c):
  r = gc.pool_regime(c)
  return r.ho, r.wo


def _sub_hw(c):
  r = gc.sub_regime(c)
  return r.ho, r.wo


@pytest.mark.parametrize('name', _names(gc.POOL))
def test_maxpool3x3_s2_f32(name):
  L, lib = _lib()
  _nhwc_case(gc.POOL, name, False, gr.pool_input, lambda c, x: gr.max_pool_3x3_s2_same(x),
             lambda c, X, Y: L.check(lib.epos_maxpool3x3_s2_f32(
                 X.ptr, c.ldx, Y.ptr, c.ldy, c.b, c.hi, c.wi, c.c, _stream()), name), _pool_hw)


@pytest.mark.parametrize('name', _names(gc.POOL_BF16))
def test_maxpool3x3_s2_bf16(name):
  L, lib = _lib()
  _nhwc_case(gc.POOL_BF16, name, True, gr.pool_input, lambda c, x: gr.max_pool_3x3_s2_same(x),
             lambda c, X, Y: L.check(lib.epos_maxpool3x3_s2_bf16(
                 X.ptr, c.ldx, Y.ptr, c.ldy, c.b, c.hi, c.wi, c.c, _stream()), name), _pool_hw)


@pytest.mark.parametrize('name', _names(gc.SUB))
def test_subsample_f32(name):
  L, lib = _lib()
  _nhwc_case(gc.SUB, name, False, gr.sub_input, lambda c, x: gr.subsample(x, c.factor),
             lambda c, X, Y: L.check(lib.epos_subsample_f32(
                 X.ptr, c.ldx, Y.ptr, c.ldy, c.b, c.hi, c.wi, c.c, c.factor, _stream()), name),
             _sub_hw)


@pytest.mark.parametrize('name', _names(gc.SUB_BF16))
def test_subsample_bf16(name):
  L, lib = _lib()
  _nhwc_case(gc.SUB_BF16, name, True, gr.sub_input, lambda c, x: gr.subsample(x, c.factor),
             lambda c, X, Y: L.check(lib.epos_subsample_bf16(
                 X.ptr, c.ldx, Y.ptr, c.ldy, c.b, c.hi, c.wi, c.c, c.factor, _stream()), name),
             _sub_hw)


# ------------------------------------------------------------------------------ add+relu ---
@pytest.mark.parametrize('name', _names(gc.ADD_RELU))
def test_add_relu_f32(name):
  L, lib = _lib()
  c = gc.by_name(gc.ADD_RELU)[name]
  a, b = gr.add_relu_input(c)

  def run():
    A, B = In(a[None], c.n, c.off), In(b[None], c.n, c.off)
    Y = Out(1, c.n, c.n, c.off)
    L.check(lib.epos_add_relu_f32(A.ptr, B.ptr, Y.ptr, c.n, _stream()), name)
    return Y.read()
  got = _f32(_twice(run)).ravel()
  assert np.array_equal(got, gr.add_relu(a, b))


@pytest.mark.parametrize('name', _names(gc.ADD_RELU_BF16))
def test_add_relu_bf16(name):
  L, lib = _lib()
  c = gc.by_name(gc.ADD_RELU_BF16)[name]
  a, b = gr.add_relu_input(c, bf16=True)

  def run():
    A, B = In(a[None], c.n, c.off, bf16=True), In(b[None], c.n, c.off, bf16=True)
    Y = Out(1, c.n, c.n, c.off, 'bf16')
    L.check(lib.epos_add_relu_bf16(A.ptr, B.ptr, Y.ptr, c.n, _stream()), name)
    return Y.read()
  got = _twice(run).view(np.uint16).ravel()
  assert np.array_equal(got, gr.add_relu_bf16_bits(a, b))


# -------------------------------------------------------------------------------- argmax ---
@pytest.mark.parametrize('name', _names(gc.ARGMAX))
def test_argmax_i64(name):
  L, lib = _lib()
  c = gc.by_name(gc.ARGMAX)[name]
  x = gr.argmax_input(c)

  def run():
    X, Y = In(x, c.ldx, c.off), Out(1, c.p, c.p, 3, 'i64')
    L.check(lib.epos_argmax_i64(X.ptr, c.ldx, Y.ptr, c.p, c.c, _stream()), name)
    return Y.read()
  got = _twice(run).ravel()
  assert np.array_equal(got, gr.argmax(x))
  assert gr.argmax_planted_ok(c, x, got)


# ------------------------------------------------------------------------------- softmax ---
def _softmax_buf(x, off):
  buf = torch.full((off + x.size + GUARD,), SENT32, dtype=torch.int32, device='cuda')
  buf[off:off + x.size] = torch.from_numpy(_bits32(x).ravel().copy()).cuda()
  assert buf.data_ptr() % 256 == 0
  return buf


def _softmax_read(buf, shape, off):
  torch.cuda.synchronize()
  raw = buf.cpu().numpy()
  n = int(np.prod(shape))
  assert (raw[:off] == SENT32).all() and (raw[off + n:] == SENT32).all(), 'stray write'
  return raw[off:off + n].reshape(shape).copy()


@pytest.mark.parametrize('name', _names(gc.SOFTMAX))
def test_softmax_groups_and_slots(name):
  """epos_softmax_groups_f32 against fp64 at the project's bound (rtol 2e-6, atol 1e-7), every
  group summing to 1 within G * 2^-23 (G > 64: G * 2^-24, the bound of test_gpu_f256.py);
  epos_softmax_slots_f32 on the same rows laid out as [B, P, O, G] gives the group form's bits
  on its slots and leaves the other groups alone."""
  L, lib = _lib()
  c = gc.by_name(gc.SOFTMAX)[name]
  x = gr.softmax_input(c)
  G, n = c.g, c.n

  def run():
    buf = _softmax_buf(x, c.off)
    L.check(lib.epos_softmax_groups_f32(_p(buf, c.off), n, G, _stream()), name)
    return _softmax_read(buf, (n, G), c.off)
  raw = _twice(run)
  dense = _f32(raw)
  np.testing.assert_allclose(dense, gr.softmax_f64(x), rtol=2e-6, atol=1e-7)
  ulp = 2.0 ** -23 if G <= 64 else 2.0 ** -24
  assert (np.abs(dense.astype(np.float64).sum(-1) - 1) <= G * ulp).all()
  B, O, P, slots = gc.softmax_slots(n)
  xs = x[:B * P * O].reshape(B, P, O, G)
  sl = torch.tensor(slots, dtype=torch.int32, device='cuda')

  def run_slots():
    buf = _softmax_buf(xs, c.off)
    L.check(lib.epos_softmax_slots_f32(_p(buf, c.off), _p(sl), len(slots), P, O, G, _stream()),
            name)
    return _softmax_read(buf, xs.shape, c.off)
  got = _twice(run_slots)
  want = raw[:B * P * O].reshape(B, P, O, G)
  for im in range(B):
    for obj in range(1, O + 1):
      src = want if (im, obj) in slots else _bits32(xs)
      assert np.array_equal(got[im, :, obj - 1], src[im, :, obj - 1]), (im, obj)


# ------------------------------------------------------------------------------- scatter ---
@pytest.mark.parametrize('name', _names(gc.SCATTER))
def test_scatter_blocks_f32(name):
  """Every float of dst outside the blocks keeps its bits (dst starts as random data between a
  sentinel lead and guard)."""
  L, lib = _lib()
  c = gc.by_name(gc.SCATTER)[name]
  dst0, offs, src = gr.scatter_problem(c)

  def run():
    D = Out(1, dst0.size, dst0.size, 4)
    D.buf[4:4 + dst0.size] = torch.from_numpy(_bits32(dst0).copy()).cuda()
    O, S = torch.from_numpy(offs).cuda(), torch.from_numpy(src).cuda()
    L.check(lib.epos_scatter_blocks_f32(D.ptr, _p(O), _p(S), c.n_blocks, c.width, _stream()),
            name)
    return D.read()
  got = _twice(run).ravel()
  assert np.array_equal(got, _bits32(gr.scatter(dst0, offs, src, c.width)))


def test_scatter_blocks_without_blocks_launches_nothing():
  L, lib = _lib()
  D = Out(1, 16, 16, 4)
  assert lib.epos_scatter_blocks_f32(D.ptr, None, None, 0, 4, _stream()) == 0
  assert (D.read() == SENT32).all()


# ----------------------------------------------------------------------- argument refusals ---
def _refused(lib, rc, fn):
  assert rc == E_INVALID, (fn, rc)
  msg = lib.epos_last_error().decode()
  assert fn in msg and len(msg) > len(fn) + 2, msg


def test_glue_launchers_refuse_invalid_arguments():
  """Every EPOS_REQUIRE of the fp32 glue launchers once: EPOS_E_INVALID, a message in
  epos_last_error() that names the function, and nothing launched (the outputs keep their
  sentinels). Among them the calls under which a kernel would leave its tensors: a pitch below
  the channel count, empty or negative sizes."""
  L, lib = _lib()
  X = In(np.zeros((2, 4, 4, 8), np.float32), 8)
  Y = Out(2 * 4 * 4, 8, 8)
  I = Out(1, 32, 32, 0, 'i64')
  x, y, s = X.ptr, Y.ptr, _stream()
  f = lib.epos_global_avg_pool_f32                       # (X, ldx, Y, B, HW, C)
  for args in [(None, 8, y, 2, 16, 8), (x, 8, None, 2, 16, 8), (x, 8, y, 2, 16, 6),
               (x, 10, y, 2, 16, 8), (x, 8, y, 2, 0, 8), (x, 8, y, 0, 16, 8), (x, 8, y, -1, 16, 8),
               (x, 8, y, 2, 16, 0), (x, 4, y, 2, 16, 8)]:
    _refused(lib, f(*args, s), 'epos_global_avg_pool_f32')
  f = lib.epos_global_avg_pool_partial_f32               # (P, ldp, Y, B, blocks, C, hw)
  for args in [(None, 8, y, 2, 4, 8, 16), (x, 8, y, 2, 4, 6, 16), (x, 4, y, 2, 4, 8, 16),
               (x, 8, y, 0, 4, 8, 16), (x, 8, y, 2, 0, 8, 16), (x, 8, y, 2, 4, 8, 0)]:
    _refused(lib, f(*args, s), 'epos_global_avg_pool_partial_f32')
  f = lib.epos_resize_bilinear_f32                       # (X, ldx, Y, ldy, B, Hi, Wi, Ho, Wo, C)
  for args in [(None, 8, y, 8, 2, 4, 4, 4, 4, 8), (x, 8, None, 8, 2, 4, 4, 4, 4, 8),
               (x, 8, y, 8, 2, 4, 4, 4, 4, 6), (x, 8, y, 10, 2, 4, 4, 4, 4, 8),
               (x, 8, y, 8, 0, 4, 4, 4, 4, 8), (x, 8, y, 8, 2, 0, 4, 4, 4, 8),
               (x, 8, y, 8, 2, 4, 0, 4, 4, 8), (x, 8, y, 8, 2, 4, 4, 0, 4, 8),
               (x, 8, y, 8, 2, 4, 4, 4, -1, 8), (x, 8, y, 8, 2, 4, 4, 4, 4, 0),
               (x, 4, y, 8, 2, 4, 4, 4, 4, 8), (x, 8, y, 4, 2, 4, 4, 4, 4, 8)]:
    _refused(lib, f(*args, s), 'epos_resize_bilinear_f32')
  f = lib.epos_maxpool3x3_s2_f32                         # (X, ldx, Y, ldy, B, Hi, Wi, C)
  for args in [(None, 8, y, 8, 2, 4, 4, 8), (x, 8, y, 8, 2, 4, 4, 6), (x, 8, y, 8, 0, 4, 4, 8),
               (x, 8, y, 8, 2, 0, 4, 8), (x, 8, y, 8, 2, 4, -2, 8), (x, 8, y, 8, 2, 4, 4, 0),
               (x, 4, y, 8, 2, 4, 4, 8), (x, 8, y, 4, 2, 4, 4, 8)]:
    _refused(lib, f(*args, s), 'epos_maxpool3x3_s2_f32')
  f = lib.epos_subsample_f32                             # (X, ldx, Y, ldy, B, Hi, Wi, C, factor)
  for args in [(x, 8, None, 8, 2, 4, 4, 8, 2), (x, 8, y, 8, 2, 4, 4, 6, 2),
               (x, 8, y, 8, 2, 4, 4, 8, 0), (x, 8, y, 8, -1, 4, 4, 8, 2),
               (x, 8, y, 8, 2, 0, 4, 8, 2), (x, 8, y, 8, 2, 4, 0, 8, 2),
               (x, 4, y, 8, 2, 4, 4, 8, 2), (x, 8, y, 4, 2, 4, 4, 8, 2)]:
    _refused(lib, f(*args, s), 'epos_subsample_f32')
  f = lib.epos_add_relu_f32                              # (A, B, Y, n)
  for args in [(None, x, y, 8), (x, None, y, 8), (x, x, None, 8), (x, x, y, 6), (x, x, y, -4)]:
    _refused(lib, f(*args, s), 'epos_add_relu_f32')
  f = lib.epos_argmax_i64                                # (X, ldx, labels, P, C)
  for args in [(None, 8, I.ptr, 4, 8), (x, 8, None, 4, 8), (x, 8, I.ptr, 4, 0),
               (x, 4, I.ptr, 4, 8), (x, 8, I.ptr, -1, 8)]:
    _refused(lib, f(*args, s), 'epos_argmax_i64')
  f = lib.epos_softmax_groups_f32                        # (X, n_groups, G)
  for args in [(None, 4, 8), (y, 4, 0), (y, 4, 257)]:
    _refused(lib, f(*args, s), 'epos_softmax_groups_f32')
  sl = torch.tensor([[0, 1]], dtype=torch.int32, device='cuda')
  f = lib.epos_softmax_slots_f32                         # (X, slots, S, P, O, F)
  for args in [(None, _p(sl), 1, 4, 1, 8), (y, None, 1, 4, 1, 8), (y, _p(sl), 1, 4, 1, 0),
               (y, _p(sl), 1, 4, 1, 257)]:
    _refused(lib, f(*args, s), 'epos_softmax_slots_f32')
  f = lib.epos_scatter_blocks_f32                        # (dst, offsets, src, n_blocks, width)
  for args in [(y, x, x, -1, 4), (y, x, x, 1, 0), (None, x, x, 1, 4), (y, None, x, 1, 4),
               (y, x, None, 1, 4)]:
    _refused(lib, f(*args, s), 'epos_scatter_blocks_f32')
  assert lib.epos_argmax_i64(x, 8, I.ptr, 0, 8, s) == 0          # P = 0: nothing to do
  assert lib.epos_add_relu_f32(x, x, y, 0, s) == 0
  assert (Y.read() == SENT32).all() and (I.read() == -1).all()


def test_bf16_glue_launchers_refuse_invalid_arguments():
  L, lib = _lib()
  X = In(np.zeros((2, 4, 4, 8), np.float32), 8, bf16=True)
  Y = Out(2 * 4 * 4, 8, 8, 0, 'bf16')
  M = Out(2, 8, 8)
  x, y, s = X.ptr, Y.ptr, _stream()
  odd_x, odd_y = _p(X.buf, 4), _p(Y.buf, 4)                # 8 bytes off: not 16-byte aligned
  f = lib.epos_resize_bilinear_bf16               # (X, ldx, x_f32, Y, ldy, B, Hi, Wi, Ho, Wo, C)
  for args in [(None, 8, 0, y, 8, 2, 4, 4, 4, 4, 8), (x, 8, 0, None, 8, 2, 4, 4, 4, 4, 8),
               (x, 8, 0, y, 8, 2, 4, 4, 4, 4, 4), (x, 8, 0, odd_y, 8, 2, 4, 4, 4, 4, 8),
               (odd_x, 8, 0, y, 8, 2, 4, 4, 4, 4, 8), (x, 8, 0, y, 8, 0, 4, 4, 4, 4, 8),
               (x, 8, 0, y, 8, 2, 0, 4, 4, 4, 8), (x, 8, 0, y, 8, 2, 4, 4, 4, 0, 8),
               (x, 8, 0, y, 8, 2, 4, 4, 4, 4, 0), (x, 0, 0, y, 8, 2, 4, 4, 4, 4, 8),
               (x, 8, 0, y, 0, 2, 4, 4, 4, 4, 8)]:
    _refused(lib, f(*args, s), 'epos_resize_bilinear_bf16')
  f = lib.epos_global_avg_pool_bf16                      # (X, ldx, Y, B, HW, C)
  for args in [(None, 8, M.ptr, 2, 16, 8), (x, 8, M.ptr, 2, 16, 4), (odd_x, 8, M.ptr, 2, 16, 8),
               (x, 8, M.ptr, 0, 16, 8), (x, 8, M.ptr, 2, 0, 8), (x, 8, M.ptr, 2, 16, 0),
               (x, 0, M.ptr, 2, 16, 8)]:
    _refused(lib, f(*args, s), 'epos_global_avg_pool_bf16')
  f = lib.epos_maxpool3x3_s2_bf16                        # (X, ldx, Y, ldy, B, Hi, Wi, C)
  for args in [(None, 8, y, 8, 2, 4, 4, 8), (x, 8, y, 8, 2, 4, 4, 4), (x, 8, odd_y, 8, 2, 4, 4, 8),
               (x, 8, y, 8, 0, 4, 4, 8), (x, 8, y, 8, 2, 0, 4, 8), (x, 8, y, 8, 2, 4, 4, 0),
               (x, 0, y, 8, 2, 4, 4, 8), (x, 8, y, 0, 2, 4, 4, 8)]:
    _refused(lib, f(*args, s), 'epos_maxpool3x3_s2_bf16')
  f = lib.epos_subsample_bf16                            # (X, ldx, Y, ldy, B, Hi, Wi, C, factor)
  for args in [(x, 8, None, 8, 2, 4, 4, 8, 2), (x, 8, y, 8, 2, 4, 4, 4, 2),
               (x, 8, y, 8, 2, 4, 4, 8, 0), (x, 8, y, 8, 0, 4, 4, 8, 2),
               (x, 8, y, 8, 2, 4, 0, 8, 2), (x, 0, y, 8, 2, 4, 4, 8, 2),
               (x, 8, y, 0, 2, 4, 4, 8, 2)]:
    _refused(lib, f(*args, s), 'epos_subsample_bf16')
  f = lib.epos_add_relu_bf16                             # (A, B, Y, n)
  for args in [(None, x, y, 8), (x, x, y, 4), (x, odd_x, y, 8), (x, x, y, -8)]:
    _refused(lib, f(*args, s), 'epos_add_relu_bf16')
  assert (Y.read() == SENT).all() and (M.read() == SENT32).all()
