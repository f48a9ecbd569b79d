"""epos_pointwise_dgrad_f32, epos_depthwise_wgrad_f32 and epos_depthwise_dgrad_f32 on the device
(csrc/pointwise_dgrad.hip, csrc/depthwise_grad.hip), through the C ABI, against
tests/helpers/decoder_backward_ref.py: to its derived bounds, or bit for bit where the
definition fixes every bit. Outputs are pre-filled with a sentinel and framed by guard words:
every element must be written and nothing around them touched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import decoder_backward_ref as ref                     # noqa: E402
from tests.helpers import pointwise_wgrad_ref as wref                     # noqa: E402
from tests.helpers.loss_device import _lib, _p, _stream                   # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = -1                               # EPOS_E_INVALID
SENT64 = 0x7FF5A5A55A5A5A5A                # NaNs no kernel produces
SENT32 = 0x7FA55A5A
GUARD = 8                                  # sentinel words in front of and behind an output
EPS = 1e-5


def _binding():
  from epos_amd import _lib as binding
  return binding


def _sent(n, dtype=torch.int32, offset=0):
  """A sentinel-filled buffer of n + 2 * GUARD words (+ offset in front, to leave the 16-byte
  alignment) and the view of its n middle words."""
  sentinel = SENT64 if dtype == torch.int64 else SENT32
  buf = torch.full((offset + n + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
  return buf, buf[offset + GUARD:offset + GUARD + n]


def _rows_written(buf, rows, width, ld, what, offset=0):
  """[rows, width] of a sentinel buffer holding rows of stride ld: every element written, the
  padding columns and the guards still sentinels; as uint32."""
  raw = buf.cpu().numpy().view(np.uint32)
  n = rows * ld
  body = raw[offset + GUARD:offset + GUARD + n].reshape(rows, ld)
  assert (raw[:offset + GUARD] == SENT32).all() and (raw[offset + GUARD + n:] == SENT32).all(), what
  assert (body[:, width:] == SENT32).all(), '%s: padding columns written' % what
  assert not (body[:, :width] == SENT32).any(), '%s: %d elements not written' % (
      what, (body[:, :width] == SENT32).sum())
  return np.ascontiguousarray(body[:, :width])


def _f64_written(buf, n, what):
  raw = buf.cpu().numpy()
  assert (raw[:GUARD] == SENT64).all() and (raw[GUARD + n:] == SENT64).all(), what
  mid = raw[GUARD:GUARD + n]
  assert not (mid == SENT64).any(), '%s: %d elements not written' % (what, (mid == SENT64).sum())
  return mid.view(np.float64)


def _padded(a, ld, offset=0):
  """a [rows, width] on the device as rows of stride ld with NaN padding, `offset` floats behind
  a 16-byte boundary: (the owning tensor, the view that starts at the data)."""
  rows, width = a.shape
  host = np.full((rows, ld), np.nan, np.float32)
  host.view(np.uint32)[:, :width] = np.ascontiguousarray(a).view(np.uint32)
  own = torch.full((offset + rows * ld,), float('nan'), device='cuda')
  own[offset:] = torch.from_numpy(host.reshape(-1)).cuda()
  return own, own[offset:]


# ====================================================== pointwise dgrad ===
class Dgrad(object):
  """One call's inputs: G [M,N], W [K,N], bn = (gamma, var) or None, mask = None, an fp32 [M,K]
  array, or ('h2', raw words [M,K]) -- fp16 pairs. pads = (ldg - N, ldm - K, ldd - K); offset:
  floats every fp32 operand lies behind a 16-byte boundary."""

  def __init__(self, G, W, bn=None, mask=None, pads=(0, 0, 0), offset=0):
    self.G, self.W, self.bn = G, W, bn
    self.M, self.N = G.shape
    self.K = W.shape[0]
    self.ldg, self.ldm, self.ldd = self.N + pads[0], self.K + pads[1], self.K + pads[2]
    self.offset = offset
    self.h2 = isinstance(mask, tuple)
    self.mask_raw = mask[1] if self.h2 else mask
    self.mask = None
    if mask is not None:
      self.mask = ref.pair_values(mask[1], self.K) if self.h2 else mask
    self.keep = [_padded(G, self.ldg, offset)]
    self.dG = self.keep[0][1]
    self.dW = torch.from_numpy(np.ascontiguousarray(W)).cuda()
    self.dbn = [torch.from_numpy(v).cuda() for v in bn] if bn else [None, None]
    self.dmask = None
    if mask is not None:
      self.keep.append(_padded(self.mask_raw, self.ldm, 0 if self.h2 else offset))
      self.dmask = self.keep[-1][1]
    nbytes = _lib().epos_pointwise_dgrad_workspace_bytes(self.K, self.N)
    assert nbytes == 8 * (-(-self.K // 64) * 64) * (-(-self.N // 16) * 16)
    self.ws = torch.empty(nbytes // 8, dtype=torch.float64, device='cuda')
    self._ref = None

  def args(self, out, **over):
    f = dict(G=_p(self.dG), ldg=self.ldg, W=_p(self.dW), gamma=_p(self.dbn[0]),
             moving_variance=_p(self.dbn[1]), eps=EPS, mask=_p(self.dmask), ldm=self.ldm,
             mask_h2=int(self.h2), M=self.M, K=self.K, N=self.N, D=_p(out), ldd=self.ldd,
             workspace=_p(self.ws))
    f.update(over)
    return _binding().PointwiseDgradArgs(**f)

  def run(self):
    """One call: D [M,K] as uint32 words, as the device wrote them."""
    lib = _lib()
    buf, D = _sent(self.M * self.ldd, offset=self.offset)
    rc = lib.epos_pointwise_dgrad_f32(ctypes.byref(self.args(D)), _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    return _rows_written(buf, self.M, self.K, self.ldd, 'D', self.offset)

  def reference(self):
    if self._ref is None:
      self.Wf = ref.fold(self.W, *(self.bn or (None, None)), eps=EPS)
      self._ref = ref.pointwise_dgrad(self.G, self.Wf, self.mask)
    return self._ref

  def check(self, bits):
    want, absum = self.reference()
    got = bits.view(np.float32)
    ok, worst = wref.within(got, want, ref.bound_pointwise_dgrad(self.N, want, absum))
    print('D M=%d K=%d N=%d mask=%s: worst error / bound = %.3g' % (
        self.M, self.K, self.N, 'h2' if self.h2 else self.mask is not None, worst))
    assert ok, worst
    if self.mask is not None:
      with np.errstate(invalid='ignore'):
        off = self.mask <= 0
      assert not bits[off].any(), 'a masked element is not +0.0'     # the BYTES of +0.0
      assert self.mask.size < 8 or (off.any() and not off.all())


def _mask_for(M, K, rng, kind):
  """None, an fp32 mask with exact zeros, -0.0 and a NaN, or the pairs of such a mask."""
  if kind == 'none':
    return None
  a = np.maximum(rng.randn(M, K), 0).astype(np.float32) * 3          # behind a ReLU
  if kind == 'f32':
    a[0, 0] = -0.0
    if M * K > 4:
      a[-1, -1] = np.nan                                              # a NaN does not mask
      a[M // 2, K // 2] = -1.5
    return a
  return ('h2', wref.h2_split(a, wref.h2_scale(np.float32(np.abs(a).max() + 1))[0]))


def random_dgrad(M, K, N, seed, kind='none', bn=True, pads=(0, 0, 0), offset=0):
  rng = np.random.RandomState(seed)
  G = (rng.randn(M, N) * rng.rand(1, N) * 1e-2).astype(np.float32)
  G[rng.rand(M, N) < 0.3] = 0.0
  W = (0.3 * rng.randn(K, N)).astype(np.float32)
  bnv = (rng.randn(N).astype(np.float32), (0.1 + rng.rand(N)).astype(np.float32)) if bn else None
  return Dgrad(G, W, bnv, _mask_for(M, K, rng, kind), pads, offset)


@pytest.mark.parametrize('kind', ['f32', 'h2'])
def test_dgrad_exact_integer_layout(kind):
  """Small integers with asymmetric patterns in p, k and c: every product and sum is exact, so D
  is compared bit for bit. A transposed or permuted tile cannot pass. Several row and column
  blocks, overhang on M, K and N."""
  M, K, N = 1001, 132, 200
  p, k, c = np.arange(M)[:, None], np.arange(K)[:, None], np.arange(N)[None, :]
  G = ((p * 5 + c * 11 + (p + 2 * c) % 7) % 17 - 9).astype(np.float32)
  W = ((k * 7 + c * 3 + (k * c) % 5) % 13 - 4).astype(np.float32)
  pm, km = np.arange(M)[:, None], np.arange(K)[None, :]
  mask = ((pm * 3 + km * 5 + (pm * km) % 7) % 4 - 1).astype(np.float32)   # -1, 0, 1, 2
  given = mask if kind == 'f32' else ('h2', wref.h2_split(mask, 2.0 ** 10))
  prob = Dgrad(G, W, None, given)
  if kind == 'h2':
    assert np.array_equal(np.sign(prob.mask), np.sign(mask))
  bits = prob.run()
  want = np.where(mask <= 0, 0.0, G.astype(np.float64) @ W.astype(np.float64).T)
  assert np.abs(want).max() < 2 ** 24
  assert np.array_equal(bits, want.astype(np.float32).view(np.uint32))


DGRAD_SHAPES = [(1, 1, 1), (63, 4, 4), (257, 20, 36), (1536, 256, 256), (1000, 256, 304),
                (20000, 8, 16)]
DGRAD_SWEEP = [(s, kind) for s in DGRAD_SHAPES for kind in ('none', 'f32', 'h2')
               if not (kind == 'h2' and s[1] % 4)]


@pytest.mark.parametrize('shape,kind', DGRAD_SWEEP,
                         ids=['x'.join(str(v) for v in s) + '-' + k for s, k in DGRAD_SWEEP])
def test_dgrad_shape_sweep_to_bound(shape, kind):
  M, K, N = shape
  prob = random_dgrad(M, K, N, seed=M + K + N, kind=kind)
  prob.check(prob.run())


@pytest.mark.parametrize('kind', ['f32', 'h2'])
def test_dgrad_padding_columns_are_never_read_or_written(kind):
  """ldg > N, ldm > K, ldd > K with NaN padding in the inputs and sentinels in D's; odd pads take
  the fp32 rows off their 16-byte alignment (the scalar loads and stores)."""
  pads = (3, 5, 7) if kind == 'f32' else (3, 4, 7)
  prob = random_dgrad(300, 20, 36, seed=9, kind=kind, pads=pads)
  bits = prob.run()
  assert np.isfinite(bits.view(np.float32)).all()
  prob.check(bits)


def test_dgrad_unaligned_operands_with_odd_sizes():
  """G, mask and D one float behind a 16-byte boundary, K and N odd: the scalar paths."""
  prob = random_dgrad(130, 7, 5, seed=4, kind='f32', offset=1)
  assert prob.dG.data_ptr() % 16 == 4 and prob.dmask.data_ptr() % 16 == 4
  prob.check(prob.run())
  prob = random_dgrad(130, 8, 12, seed=5, kind='f32', offset=1)       # even sizes, unaligned
  prob.check(prob.run())


def test_dgrad_fold():
  """A batch norm with a zero gamma, negative gammas and a tiny variance, and none at all: Wf is
  rebuilt on the host exactly as the plan's fold does it (scale in fp64 rounded to fp32, then one
  fp32 product), and D must lie within the bound of THAT matrix."""
  M, K, N = 200, 24, 40
  rng = np.random.RandomState(3)
  G = (rng.randn(M, N) * 1e-2).astype(np.float32)
  W = (0.3 * rng.randn(K, N)).astype(np.float32)
  gamma = rng.randn(N).astype(np.float32)
  gamma[1] = 0.0
  gamma[2:6] = -np.abs(gamma[2:6]) - 0.5
  var = (0.1 + rng.rand(N)).astype(np.float32)
  var[7] = 1e-12                                                       # scale ~ gamma / sqrt(eps)
  prob = Dgrad(G, W, (gamma, var), _mask_for(M, K, rng, 'f32'))
  prob.check(prob.run())
  scale = (gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + EPS)).astype(np.float32)
  assert np.array_equal(prob.Wf, W * scale[None, :]) and prob.Wf.dtype == np.float32
  assert abs(scale[7]) > 100 * abs(gamma[7]) and not prob.Wf[:, 1].any()
  # folding in fp64 instead gives another matrix: the test would see the difference
  assert (prob.Wf.astype(np.float64) != W.astype(np.float64) * scale.astype(np.float64)).any()
  plain = Dgrad(G, W, None, prob.mask_raw)
  bits = plain.run()
  plain.check(bits)
  assert np.array_equal(plain.Wf, W)


def test_dgrad_mask_from_the_depthwise_kernels_own_pairs():
  """mask = what epos_depthwise3x3_f32 writes with y_h2 = 1; the reference reads the sign of the
  bytes the device wrote, and must agree with the sign of the fp32 output except where the split
  flushed a tiny positive value to zero."""
  binding = _binding()
  lib = _lib()
  B, H, Wd, C, N = 2, 12, 16, 40, 24
  rng = np.random.RandomState(21)
  x = rng.randn(B, H, Wd, C).astype(np.float32)
  w9c = (0.5 * rng.randn(9, C)).astype(np.float32)
  bias = rng.randn(C).astype(np.float32)
  gain = float(np.abs(w9c.astype(np.float64)).sum(0).max())
  bias0 = float(np.abs(bias).max())
  slot = np.zeros(64, np.uint32)
  slot[9] = np.float32(np.abs(x).max()).view(np.uint32)
  dslot = torch.from_numpy(slot.view(np.int32)).cuda()
  dx, dw, db = (torch.from_numpy(v).cuda() for v in (x, w9c, bias))
  y = torch.full((B * H * Wd, C), SENT32, dtype=torch.int32, device='cuda')
  args = binding.DepthwiseArgs(X=_p(dx), ldx=C, w9c=_p(dw), bias=_p(db), Y=_p(y), ldy=C, B=B,
                               Hi=H, Wi=Wd, Ho=H, Wo=Wd, C=C, stride=1, rate=1, relu_in=0,
                               relu_out=1, y_h2=1, x_amax=_p(dslot), x_amax2=None, gain=gain,
                               bias0=bias0)
  assert lib.epos_depthwise3x3_f32(ctypes.byref(args), _stream()) == 0, lib.epos_last_error()
  torch.cuda.synchronize()
  raw = y.cpu().numpy().view(np.float32)
  M = B * H * Wd
  G = (rng.randn(M, N) * 1e-2).astype(np.float32)
  W = (0.3 * rng.randn(C, N)).astype(np.float32)
  prob = Dgrad(G, W, None, ('h2', raw))
  fwd = ref.depthwise_forward(x, w9c, bias, 1).reshape(M, C)
  on = prob.mask > 0
  assert 0.3 < on.mean() < 0.7 and not (on & (fwd <= 0)).any()
  assert ((fwd > 0) & ~on).sum() <= 0.001 * M * C                      # flushed, if any
  prob.dmask = y.view(torch.float32)                                   # the device's own buffer
  prob.check(prob.run())


def test_dgrad_non_finite_values_stay_in_their_row_or_column():
  M, K, N = 300, 24, 40
  prob = random_dgrad(M, K, N, seed=15, bn=False)
  base = prob.run()
  G = prob.G.copy()
  G[201, 17] = np.nan
  G[5, 3] = np.inf
  bad = Dgrad(G, prob.W).run().view(np.float32)
  rows = np.zeros(M, bool)
  rows[[201, 5]] = True
  assert not np.isfinite(bad[rows]).any()
  assert np.array_equal(bad[~rows].view(np.uint32), base[~rows])
  W = prob.W.copy()
  W[11, 30] = np.nan
  bad = Dgrad(prob.G, W).run().view(np.float32)
  cols = np.arange(K) == 11
  assert np.isnan(bad[:, cols]).all()
  assert np.array_equal(bad[:, ~cols].view(np.uint32), base[:, ~cols])


def test_dgrad_is_deterministic_and_a_row_does_not_depend_on_its_position():
  for kind in ('none', 'h2'):
    prob = random_dgrad(1000, 256, 256, seed=12, kind=kind)
    one, two = prob.run(), prob.run()
    assert np.array_equal(one, two)
    lo, hi = 333, 471                                                 # rows alone
    part = Dgrad(prob.G[lo:hi], prob.W, prob.bn,
                 None if prob.mask_raw is None else ('h2', prob.mask_raw[lo:hi]))
    assert np.array_equal(part.run(), one[lo:hi])
    single = Dgrad(prob.G[lo:lo + 1], prob.W, prob.bn,
                   None if prob.mask_raw is None else ('h2', prob.mask_raw[lo:lo + 1]))
    assert np.array_equal(single.run(), one[lo:lo + 1])


def test_dgrad_graph_capture_replays_to_the_eager_bytes():
  lib = _lib()
  prob = random_dgrad(700, 64, 72, seed=8, kind='h2')
  eager = prob.run()
  D = torch.zeros(prob.M * prob.ldd, device='cuda')
  args = prob.args(D)

  def enqueue():
    assert lib.epos_pointwise_dgrad_f32(ctypes.byref(args), _stream()) == 0
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    enqueue()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    enqueue()
  D.fill_(-1.0)
  prob.ws.fill_(-1.0)                                                  # the fold is replayed too
  graph.replay()
  torch.cuda.synchronize()
  assert np.array_equal(D.cpu().numpy().view(np.uint32).reshape(prob.M, prob.K), eager)


def test_dgrad_refusals_leave_the_sentinels():
  lib = _lib()
  f32 = random_dgrad(300, 20, 36, seed=1, kind='f32', pads=(0, 4, 0))
  h2 = random_dgrad(300, 20, 36, seed=1, kind='h2', pads=(0, 4, 0))
  pairs = b'a pre-split mask needs K % 4 == 0, ldm % 4 == 0 and 16-byte aligned rows'
  together = b'gamma and moving_variance are given together or not at all'
  cases = [(f32, dict(G=None), b'null pointer'), (f32, dict(W=None), b'null pointer'),
           (f32, dict(workspace=None), b'null pointer'),
           (f32, dict(M=0), b'M, K and N must be positive'),
           (f32, dict(K=0), b'M, K and N must be positive'),
           (f32, dict(N=1025), b'K and N must be in 1..1024'),
           (f32, dict(ldg=35), b'ldg must be >= N'), (f32, dict(ldd=19), b'ldd must be >= K'),
           (f32, dict(ldm=19), b'ldm must be >= K'),
           (f32, dict(gamma=None), together), (f32, dict(moving_variance=None), together),
           (f32, dict(eps=-1.0), b'eps must be a non-negative number'),
           (f32, dict(eps=float('nan')), b'eps must be a non-negative number'),
           (f32, dict(G=ctypes.c_void_p(f32.dG.data_ptr() + 2)), None),
           (h2, dict(ldm=22), pairs), (h2, dict(K=18), pairs),
           (h2, dict(mask=ctypes.c_void_p(h2.dmask.data_ptr() + 4)), pairs),
           (f32, dict(mask=None, D=_p(f32.dG)), b'D may not start at G or at mask')]
  for prob, over, msg in cases:
    buf, D = _sent(prob.M * prob.ldd)
    rc = lib.epos_pointwise_dgrad_f32(ctypes.byref(prob.args(D, **over)), _stream())
    assert rc == INVALID, over
    if msg is not None:
      assert lib.epos_last_error() == b'epos_pointwise_dgrad_f32: ' + msg, over
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == SENT32).all(), over
  buf, D = _sent(f32.M * f32.ldd)
  args = f32.args(D, mask=_p(D))
  assert lib.epos_pointwise_dgrad_f32(ctypes.byref(args), _stream()) == INVALID
  assert lib.epos_pointwise_dgrad_f32(None, _stream()) == INVALID
  assert (buf.cpu().numpy().view(np.uint32) == SENT32).all()
  assert not np.isnan(f32.dG[:f32.M * f32.ldg].cpu().numpy().reshape(f32.M, -1)[:, :36]).any()


# ============================================================ depthwise ===
class Depthwise(object):
  """X and D [B,H,W,C] on the device with pixel strides C + pads and NaN padding."""

  def __init__(self, X, D, rate, pads=(0, 0)):
    self.X, self.D, self.rate = X, D, rate
    self.B, self.H, self.W, self.C = X.shape
    self.P = self.B * self.H * self.W
    self.ldx, self.ldd = self.C + pads[0], self.C + pads[1]
    self.keep = [_padded(X.reshape(self.P, self.C), self.ldx),
                 _padded(D.reshape(self.P, self.C), self.ldd)]
    self.dX, self.dD = self.keep[0][1], self.keep[1][1]
    lib = _lib()
    dims = (self.B, self.H, self.W, self.C)
    self.range = lib.epos_depthwise_wgrad_range_pixels(*dims)
    self.ranges = -(-self.P // self.range)
    nbytes = lib.epos_depthwise_wgrad_workspace_bytes(*dims)
    assert nbytes == (0 if self.ranges == 1 else self.ranges * 80 * self.C)
    self.ws = torch.empty(max(1, nbytes // 8), dtype=torch.int64, device='cuda')
    self._ref = None

  def wgrad_args(self, out_T, out_t, **over):
    f = dict(X=_p(self.dX), ldx=self.ldx, D=_p(self.dD), ldd=self.ldd, B=self.B, H=self.H,
             W=self.W, C=self.C, stride=1, rate=self.rate, T=_p(out_T), t=_p(out_t),
             workspace=_p(self.ws))
    f.update(over)
    return _binding().DepthwiseWgradArgs(**f)

  def wgrad(self):
    """One call: (T f64 [9,C], t f64 [C]) as the device wrote them."""
    lib = _lib()
    bT, T = _sent(9 * self.C, torch.int64)
    bt, t = _sent(self.C, torch.int64)
    rc = lib.epos_depthwise_wgrad_f32(ctypes.byref(self.wgrad_args(T, t)), _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    return (_f64_written(bT, 9 * self.C, 'T').reshape(9, self.C).copy(),
            _f64_written(bt, self.C, 't').copy())

  def reference(self):
    if self._ref is None:
      self._ref = ref.depthwise_wgrad(self.X, self.D, self.rate)
    return self._ref

  def check_wgrad(self, T, t):
    rT, rt, aT, at = self.reference()
    for got, want, a, what in ((T, rT, aT, 'T'), (t, rt, at, 't')):
      ok, worst = wref.within(got, want, ref.bound_depthwise_wgrad(self.P, a))
      print('%s %dx%dx%dx%d rate=%d ranges=%d: worst error / bound = %.3g' % (
          what, self.B, self.H, self.W, self.C, self.rate, self.ranges, worst))
      assert ok, (what, worst)

  def dgrad(self, weights, Y=None, ldy_pad=0, ldx_pad=0, **over):
    """epos_depthwise_dgrad_f32 on D: dX [B,H,W,C] as uint32 words (None when refused, after the
    sentinel check)."""
    lib = _lib()
    dw = torch.from_numpy(np.ascontiguousarray(weights)).cuda()
    ldy, ldo = self.C + ldy_pad, self.C + ldx_pad
    dY = _padded(Y.reshape(self.P, self.C), ldy)[1] if Y is not None else None
    buf, out = _sent(self.P * ldo)
    f = dict(D=_p(self.dD), ldd=self.ldd, w9c=_p(dw), Y=_p(dY), ldy=ldy, dX=_p(out), ldx=ldo,
             B=self.B, H=self.H, W=self.W, C=self.C, rate=self.rate)
    f.update(over)
    rc = lib.epos_depthwise_dgrad_f32(f['D'], f['ldd'], f['w9c'], f['Y'], f['ldy'], f['dX'],
                                      f['ldx'], f['B'], f['H'], f['W'], f['C'], f['rate'],
                                      _stream())
    torch.cuda.synchronize()
    if rc != 0:
      assert rc == INVALID and (buf.cpu().numpy().view(np.uint32) == SENT32).all(), over
      return None
    return _rows_written(buf, self.P, self.C, ldo, 'dX').reshape(self.B, self.H, self.W, self.C)


def random_depthwise(B, H, Wd, C, rate, seed, pads=(0, 0)):
  rng = np.random.RandomState(seed)
  X = np.maximum(rng.randn(B, H, Wd, C), 0).astype(np.float32) * 2    # behind a ReLU
  D = (rng.randn(B, H, Wd, C) * 1e-2).astype(np.float32)
  D[rng.rand(B, H, Wd, C) < 0.4] = 0.0                                # the ReLU mask's zeros
  return Depthwise(X, D, rate, pads)


DW_SHAPES = [(1, 1, 1, 4), (2, 3, 5, 4), (2, 12, 16, 40), (1, 30, 40, 256), (1, 80, 81, 8)]
DW_SWEEP = [(s, r) for s in DW_SHAPES for r in (1, 3)]
DW_IDS = ['x'.join(str(v) for v in s) + '-rate%d' % r for s, r in DW_SWEEP]


def test_depthwise_wgrad_exact_integer_layout():
  """Small integers, H != W, two different images, more than one range: bit-equal. X and D depend
  on b, y, x and c through different non-symmetric expressions, so swapping ky and kx, flipping a
  tap or reading across the image boundary changes T."""
  B, H, Wd, C = 2, 9, 14, 8
  b, y = np.arange(B)[:, None, None, None], np.arange(H)[None, :, None, None]
  x, c = np.arange(Wd)[None, None, :, None], np.arange(C)[None, None, None, :]
  X = ((b * 5 + y * 7 + x * 3 + c + (x * y) % 5) % 11 - 3).astype(np.float32)
  D = ((b * 3 + y * 2 + x * 5 + c * 7 + (y + 2 * x) % 3) % 13 - 6).astype(np.float32)
  for rate in (1, 2):
    prob = Depthwise(X, D, rate)
    assert prob.ranges > 1
    T, t = prob.wgrad()
    rT, rt, _, _ = prob.reference()
    assert np.array_equal(T.view(np.uint64), rT.view(np.uint64))
    assert np.array_equal(t.view(np.uint64), rt.view(np.uint64))
    # the pattern tells the mistakes apart
    Xt = np.ascontiguousarray(X.transpose(0, 2, 1, 3))
    Dt = np.ascontiguousarray(D.transpose(0, 2, 1, 3))
    swapped = ref.depthwise_wgrad(Xt, Dt, rate)[0].reshape(3, 3, C).transpose(1, 0, 2)
    assert np.array_equal(swapped.reshape(9, C), rT)                  # the restatement's own check
    assert not np.array_equal(rT.reshape(3, 3, C).transpose(1, 0, 2).reshape(9, C), rT)
    assert not np.array_equal(rT[::-1], rT)
    one = ref.depthwise_wgrad(X.reshape(1, B * H, Wd, C), D.reshape(1, B * H, Wd, C), rate)[0]
    assert not np.array_equal(one, rT)                                # a leak across the images


@pytest.mark.parametrize('shape,rate', DW_SWEEP, ids=DW_IDS)
def test_depthwise_wgrad_shape_sweep_to_bound(shape, rate):
  """ldx > C and ldd > C with NaN padding throughout."""
  prob = random_depthwise(*shape, rate=rate, seed=sum(shape) + rate, pads=(4, 8))
  if shape == (1, 80, 81, 8):
    assert prob.ranges > 100
  if shape[1] * shape[2] < 64:
    assert prob.ranges == 1                                            # written directly
  T, t = prob.wgrad()
  assert np.isfinite(T).all() and np.isfinite(t).all()
  prob.check_wgrad(T, t)
  if rate == 3 and shape[1] <= 3:
    assert not T[:3].any() and not T[6:].any()       # every off-centre row tap is in the padding


@pytest.mark.parametrize('C', [256, 40])
def test_depthwise_closing_through_the_pointwise_entry(C):
  """epos_pointwise_wgrad_close_f32 with K = 9 on the device's T and t against the restatement,
  to that entry's own bound."""
  from tests.test_gpu_pointwise_wgrad import close, random_bn
  prob = random_depthwise(2, 12, 16, C, rate=1, seed=C)
  T, t = prob.wgrad()
  rT, rt, aT, at = prob.reference()
  rng = np.random.RandomState(C)
  w = (0.5 * rng.randn(9, C)).astype(np.float32)
  bn = random_bn(C, seed=C + 1)
  rc, dw, dgamma, dbeta = close(T, t, w, bn)
  assert rc == 0
  want = wref.close(rT, rt, w, *bn, eps=EPS)
  tol = wref.bounds_close(prob.P, rT, rt, aT, at, w, *bn, eps=EPS)
  for got, wv, tv, what in zip((dw, dgamma, dbeta), want, tol, ('dw', 'dgamma', 'dbeta')):
    ok, worst = wref.within(got, wv, tv)
    print('%s C=%d: worst error / bound = %.3g' % (what, C, worst))
    assert ok, (what, worst)
  assert np.abs(dw).max() > 0 and np.abs(dgamma).max() > 0


def test_depthwise_wgrad_zero_gradient_gives_positive_zero_bytes():
  prob = random_depthwise(2, 12, 16, 40, rate=1, seed=6)
  zero = Depthwise(-np.abs(prob.X) - 1, np.zeros_like(prob.D), 1)
  assert zero.ranges > 1
  T, t = zero.wgrad()
  assert not T.view(np.uint64).any() and not t.view(np.uint64).any()


def test_depthwise_wgrad_is_deterministic_and_graph_capture_replays_it():
  lib = _lib()
  prob = random_depthwise(2, 30, 40, 64, rate=2, seed=12)
  assert prob.ranges > 1
  T1, t1 = prob.wgrad()
  T2, t2 = prob.wgrad()
  assert np.array_equal(T1.view(np.uint64), T2.view(np.uint64))
  assert np.array_equal(t1.view(np.uint64), t2.view(np.uint64))
  T = torch.zeros(9 * prob.C, dtype=torch.float64, device='cuda')
  t = torch.zeros(prob.C, dtype=torch.float64, device='cuda')
  args = prob.wgrad_args(T, t)

  def enqueue():
    assert lib.epos_depthwise_wgrad_f32(ctypes.byref(args), _stream()) == 0
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    enqueue()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    enqueue()
  T.fill_(-1.0)
  t.fill_(-1.0)
  graph.replay()
  torch.cuda.synchronize()
  assert np.array_equal(T.cpu().numpy().view(np.uint64).reshape(9, -1), T1.view(np.uint64))
  assert np.array_equal(t.cpu().numpy().view(np.uint64), t1.view(np.uint64))


def test_depthwise_wgrad_refusals_leave_the_sentinels():
  lib = _lib()
  prob = random_depthwise(2, 12, 16, 40, rate=1, seed=1)
  assert prob.ranges > 1
  aligned = b'X and D must be 16-byte aligned, T and t 8-byte aligned'
  for over, msg in ((dict(X=None), b'null pointer'), (dict(D=None), b'null pointer'),
                    (dict(B=0), b'B, H, W and C must be positive'),
                    (dict(C=38), b'C must be a multiple of 4'),
                    (dict(stride=2), b'stride must be 1'), (dict(rate=0), b'rate must be >= 1'),
                    (dict(ldx=36), b'ldx must be >= C and a multiple of 4'),
                    (dict(ldd=42), b'ldd must be >= C and a multiple of 4'),
                    (dict(X=ctypes.c_void_p(prob.dX.data_ptr() + 4)), aligned),
                    (dict(workspace=None), b'the workspace must be given, 8-byte aligned')):
    bT, T = _sent(9 * prob.C, torch.int64)
    bt, t = _sent(prob.C, torch.int64)
    rc = lib.epos_depthwise_wgrad_f32(ctypes.byref(prob.wgrad_args(T, t, **over)), _stream())
    assert rc == INVALID, over
    assert lib.epos_last_error() == b'epos_depthwise_wgrad_f32: ' + msg, over
    torch.cuda.synchronize()
    assert (bT.cpu().numpy() == SENT64).all() and (bt.cpu().numpy() == SENT64).all(), over
  bT, T = _sent(9 * prob.C, torch.int64)
  for over in (dict(T=None), dict(t=None)):
    assert lib.epos_depthwise_wgrad_f32(ctypes.byref(prob.wgrad_args(T, T, **over)),
                                        _stream()) == INVALID
  assert (bT.cpu().numpy() == SENT64).all()


@pytest.mark.parametrize('shape,rate', DW_SWEEP, ids=DW_IDS)
def test_depthwise_dgrad_is_bit_equal_to_the_restatement(shape, rate):
  """With and without the mask; pixel strides wider than C on every operand."""
  prob = random_depthwise(*shape, rate=rate, seed=sum(shape) + 7 * rate, pads=(0, 4))
  rng = np.random.RandomState(rate)
  w9c = (0.5 * rng.randn(9, prob.C)).astype(np.float32)
  got = prob.dgrad(w9c, ldx_pad=8)
  assert np.array_equal(got, ref.depthwise_dgrad(prob.D, w9c, rate).view(np.uint32))
  Y = prob.X.copy()
  Y.reshape(-1)[0] = -0.0
  if Y.size > 8:
    Y.reshape(-1)[5] = np.nan
  got = prob.dgrad(w9c, Y=Y, ldy_pad=4, ldx_pad=8)
  want = ref.depthwise_dgrad(prob.D, w9c, rate, Y=Y)
  assert np.array_equal(got, want.view(np.uint32))
  with np.errstate(invalid='ignore'):
    assert not got[Y <= 0].any()                                       # the BYTES of +0.0


def test_depthwise_dgrad_an_image_does_not_depend_on_its_position():
  rng = np.random.RandomState(5)
  w9c = (0.5 * rng.randn(9, 40)).astype(np.float32)
  batch = random_depthwise(3, 12, 16, 40, rate=2, seed=3)
  alone = Depthwise(batch.X[1:2], batch.D[1:2], 2)
  got = batch.dgrad(w9c, Y=batch.X)
  assert np.array_equal(alone.dgrad(w9c, Y=alone.X)[0], got[1])
  assert np.array_equal(got, batch.dgrad(w9c, Y=batch.X))             # and the same in every run


def test_depthwise_dgrad_a_nan_reaches_exactly_its_neighbours():
  B, H, Wd, C, rate = 2, 9, 11, 8, 2
  prob = random_depthwise(B, H, Wd, C, rate=rate, seed=2)
  rng = np.random.RandomState(9)
  w9c = (0.5 * rng.randn(9, C)).astype(np.float32)
  w9c[4, 3] = 0.0                                                      # 0 * NaN is a NaN too
  base = prob.dgrad(w9c)
  D = prob.D.copy()
  D[1, 4, 5, 3] = np.nan                                               # nine neighbours
  D[0, 0, 10, 6] = np.nan                                              # a corner: four
  got = Depthwise(prob.X, D, rate).dgrad(w9c).view(np.float32)
  hit = np.zeros((B, H, Wd, C), bool)
  for (b, y, x, c) in ((1, 4, 5, 3), (0, 0, 10, 6)):
    for dy in (-rate, 0, rate):
      for dx in (-rate, 0, rate):
        if 0 <= y + dy < H and 0 <= x + dx < Wd:
          hit[b, y + dy, x + dx, c] = True
  assert hit.sum() == 9 + 4
  assert np.isnan(got[hit]).all()
  assert np.array_equal(got.view(np.uint32)[~hit], base[~hit])


def test_depthwise_dgrad_refusals_leave_the_sentinels():
  lib = _lib()
  prob = random_depthwise(1, 4, 6, 8, rate=1, seed=1)
  w9c = np.ones((9, 8), np.float32)
  for over, msg in ((dict(D=None), b'null pointer'), (dict(w9c=None), b'null pointer'),
                    (dict(B=0), b'B, H, W and C must be positive'),
                    (dict(C=6), b'C must be a multiple of 4'),
                    (dict(rate=0), b'rate must be >= 1'),
                    (dict(ldd=4), b'ldd must be >= C and a multiple of 4'),
                    (dict(ldx=10), b'ldx must be >= C and a multiple of 4'),
                    (dict(ldy=9), b'ldy must be >= C and a multiple of 4'),
                    (dict(D=ctypes.c_void_p(prob.dD.data_ptr() + 4)),
                     b'D, w9c, Y and dX must be 16-byte aligned')):
    assert prob.dgrad(w9c, Y=prob.X, **over) is None, over
    assert lib.epos_last_error() == b'epos_depthwise_dgrad_f32: ' + msg, over
  d = prob.dD
  rc = lib.epos_depthwise_dgrad_f32(_p(d), 8, _p(d), None, 8, _p(d), 8, 1, 4, 6, 8, 1, _stream())
  assert rc == INVALID
  assert lib.epos_last_error() == b'epos_depthwise_dgrad_f32: dX may not start at D'
  assert lib.epos_depthwise_dgrad_f32(_p(d), 8, _p(d), None, 8, None, 8, 1, 4, 6, 8, 1,
                                      _stream()) == INVALID
