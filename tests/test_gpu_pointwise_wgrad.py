"""epos_pointwise_wgrad_f32 and epos_pointwise_wgrad_close_f32 on the device
(csrc/pointwise_wgrad.hip), through the C ABI, against tests/helpers/pointwise_wgrad_ref.py to
its derived bounds. Outputs are pre-filled with a sentinel: every element must be written and
nothing around them touched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import pointwise_wgrad_ref as ref                      # noqa: E402
from tests.helpers.loss_device import _lib, _p, _stream                   # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = -1                               # EPOS_E_INVALID
SENT64 = 0x7FF5A5A55A5A5A5A                # a NaN no kernel produces
SENT32 = 0x7FA55A5A
GUARD = 8                                  # sentinel words in front of and behind an output
EPS = 1e-5


def _sent(n, dtype):
  """A sentinel-filled buffer of n + 2 * GUARD words and the view of its n middle words."""
  sentinel = SENT64 if dtype == torch.int64 else SENT32
  buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
  return buf, buf[GUARD:GUARD + n]


def _check_sent(buf, n, what):
  """The middle words all written, the guards untouched; returns the middle as numpy."""
  raw = buf.cpu().numpy()
  sentinel = SENT64 if raw.dtype == np.int64 else SENT32
  assert (raw[:GUARD] == sentinel).all() and (raw[GUARD + n:] == sentinel).all(), what
  mid = raw[GUARD:GUARD + n]
  assert not (mid == sentinel).any(), '%s: %d elements not written' % (
      what, (mid == sentinel).sum())
  return mid


def _slot(bound, word=5):
  s = np.zeros(64, np.uint32)
  s[word] = np.float32(bound).view(np.uint32)
  return s


class Problem(object):
  """One call's inputs. A [M,K] and G [M,N] fp32 on the host; lda / ldg with NaN padding; h2 =
  None (fp32 A) or (slot, slot2 or None, gain, bias): A goes to the device as the fp16 pairs
  ref.h2_split writes at the slots' scale, and the reference reads those bytes back."""

  def __init__(self, A, G, lda=None, ldg=None, h2=None, raw=None):
    from epos_amd import _lib as binding
    self.M, self.K = A.shape
    self.N = G.shape[1]
    self.lda, self.ldg = lda or self.K, ldg or self.N
    self.h2 = h2
    words = np.full((self.M, self.lda), np.nan, np.float32)
    bits = words.view(np.uint32)             # copied as integers: the pairs are no floats
    if raw is not None:                      # fp16 pairs a device kernel wrote
      bits[:, :self.K] = raw.view(np.uint32)
      self.A64 = ref.h2_values(raw, self.K, ref.h2_scale(ref.slot_bound(*h2))[1])
    elif h2 is not None:
      s, inv = ref.h2_scale(ref.slot_bound(*h2))
      bits[:, :self.K] = ref.h2_split(A, s).view(np.uint32)
      self.A64 = ref.h2_values(words, self.K, inv)
    else:
      words[:, :self.K] = A
      self.A64 = A.astype(np.float64)
    gw = np.full((self.M, self.ldg), np.nan, np.float32)
    gw[:, :self.N] = G
    self.G = G
    self.dA = torch.from_numpy(words.view(np.int32)).cuda()     # bytes, whatever they mean
    self.dG = torch.from_numpy(gw).cuda()
    self.slots = [None, None]
    if h2 is not None:
      self.slots[0] = torch.from_numpy(h2[0].view(np.int32)).cuda()
      if h2[1] is not None:
        self.slots[1] = torch.from_numpy(h2[1].view(np.int32)).cuda()
    lib = _lib()
    nbytes = lib.epos_pointwise_wgrad_workspace_bytes(self.M, self.K, self.N)
    assert nbytes >= 0
    self.rows = lib.epos_pointwise_wgrad_range_rows(self.M, self.K, self.N)
    self.ranges = -(-self.M // self.rows)
    assert nbytes == (0 if self.ranges == 1 else self.ranges * 8 * (self.K * self.N + self.N))
    self.ws = torch.empty(max(1, nbytes // 8), dtype=torch.int64, device='cuda')
    self.binding = binding
    self._ref = None

  def args(self, out_S, out_g, **over):
    f = dict(A=_p(self.dA), lda=self.lda, G=_p(self.dG), ldg=self.ldg, M=self.M, K=self.K,
             N=self.N, a_presplit=int(self.h2 is not None), a_amax=_p(self.slots[0]),
             a_amax2=_p(self.slots[1]), a_gain=self.h2[2] if self.h2 else 0.0,
             a_bias=self.h2[3] if self.h2 else 0.0, S=_p(out_S), g=_p(out_g),
             workspace=_p(self.ws))
    f.update(over)
    return self.binding.PointwiseWgradArgs(**f)

  def run(self):
    """One call: (S f64 [K,N], g f64 [N]) as the device wrote them."""
    lib = _lib()
    bS, S = _sent(self.K * self.N, torch.int64)
    bg, g = _sent(self.N, torch.int64)
    rc = lib.epos_pointwise_wgrad_f32(ctypes.byref(self.args(S, g)), _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    S = _check_sent(bS, self.K * self.N, 'S').view(np.float64).reshape(self.K, self.N)
    g = _check_sent(bg, self.N, 'g').view(np.float64)
    return S, g

  def reference(self):
    if self._ref is None:
      self._ref = ref.sums(self.A64, self.G)
    return self._ref

  def check(self, S, g):
    rS, rg, aS, ag = self.reference()
    for got, want, a, what in ((S, rS, aS, 'S'), (g, rg, ag, 'g')):
      ok, worst = ref.within(got, want, ref.bound(self.M, np.where(np.isfinite(a), a, 0.0)))
      print('%s M=%d K=%d N=%d ranges=%d: worst error / bound = %.3g' % (
          what, self.M, self.K, self.N, self.ranges, worst))
      assert ok, (what, worst)


def close(hS, hg, hW=None, bn=None, K=None, N=None, **over):
  """epos_pointwise_wgrad_close_f32 on host arrays: (rc, dW, dgamma or None, dbeta) as the device
  wrote them (None for all three when the call is refused, after the sentinel check)."""
  lib = _lib()
  K, N = hS.shape[0] if K is None else K, hS.shape[1] if N is None else N
  dS = torch.from_numpy(np.ascontiguousarray(hS)).cuda()
  dg = torch.from_numpy(np.ascontiguousarray(hg)).cuda()
  dWt = torch.from_numpy(hW).cuda() if hW is not None else None
  bnd = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for v in bn] if bn else \
      [None] * 3
  bW, oW = _sent(hS.size, torch.int32)
  bga, oga = _sent(hS.shape[1], torch.int32)
  bbe, obe = _sent(hS.shape[1], torch.int32)
  a = dict(S=_p(dS), g=_p(dg), W=_p(dWt), gamma=_p(bnd[0]), mean=_p(bnd[1]), var=_p(bnd[2]),
           eps=EPS, dW=_p(oW), dgamma=_p(oga) if bn else None, dbeta=_p(obe))
  a.update(over)
  rc = lib.epos_pointwise_wgrad_close_f32(a['S'], a['g'], a['W'], K, N, a['gamma'], a['mean'],
                                          a['var'], a['eps'], a['dW'], a['dgamma'], a['dbeta'],
                                          _stream())
  torch.cuda.synchronize()
  if rc != 0:
    for b in (bW, bga, bbe):
      assert (b.cpu().numpy() == SENT32).all()
    return rc, None, None, None
  dW = _check_sent(bW, hS.size, 'dW').view(np.float32).reshape(hS.shape)
  dbeta = _check_sent(bbe, hS.shape[1], 'dbeta').view(np.float32)
  if bn:
    dgamma = _check_sent(bga, hS.shape[1], 'dgamma').view(np.float32)
  else:
    assert (bga.cpu().numpy() == SENT32).all()
    dgamma = None
  return rc, dW, dgamma, dbeta


def random_problem(M, K, N, seed, h2=False, pad=(0, 0)):
  rng = np.random.RandomState(seed)
  A = np.maximum(rng.randn(M, K), 0).astype(np.float32) * 3       # behind a ReLU, as the layer's
  G = (rng.randn(M, N) * rng.rand(1, N) * 1e-3).astype(np.float32)
  G[rng.rand(M, N) < 0.3] = 0.0                                   # the ReLU mask's zeros
  slots = None
  if h2:
    amax = float(np.abs(A).max())
    # two slots, the larger bound in the second, with a gain and a bias
    slots = (_slot(amax / 8, 3), _slot(amax / 2, 40), 1.75, 0.25 * amax)
    assert float(ref.slot_bound(*slots)) >= amax
  return Problem(A, G, lda=K + pad[0], ldg=N + pad[1], h2=slots)


def random_bn(N, seed, zero_gamma=1):
  rng = np.random.RandomState(seed)
  gamma = rng.randn(N).astype(np.float32)
  gamma[zero_gamma % N] = 0.0
  return gamma, rng.randn(N).astype(np.float32), (0.1 + rng.rand(N)).astype(np.float32)


# --------------------------------------------------------------- layout ---
@pytest.mark.parametrize('h2', [False, True], ids=['fp32', 'h2'])
def test_exact_integer_layout(h2):
  """Small integers with asymmetric patterns: every product and sum is exact, so S and g are
  compared bit for bit. A transposed, row-permuted or column-permuted accumulator cannot pass:
  A[p,k] and G[p,c] depend on p, k and c through different, non-symmetric expressions. More than
  one 128-block both ways, overhang on M, K and N, several row ranges."""
  M, K, N = 1001, 132, 200
  p, k, c = np.arange(M)[:, None], np.arange(K)[None, :], np.arange(N)[None, :]
  A = ((p * 7 + k * 3 + (p * k) % 5) % 13 - 4).astype(np.float32)
  G = ((p * 5 + c * 11 + (p + 2 * c) % 7) % 17 - 9).astype(np.float32)
  slots = (_slot(8.0), None, 0.0, 0.0) if h2 else None
  prob = Problem(A, G, h2=slots)
  assert prob.ranges > 1
  if h2:
    assert np.array_equal(prob.A64, A.astype(np.float64))         # integers survive the split
  S, g = prob.run()
  rS = A.astype(np.float64).T @ G.astype(np.float64)
  rg = G.astype(np.float64).sum(axis=0)
  assert np.array_equal(S.view(np.uint64), rS.view(np.uint64))
  assert np.array_equal(g.view(np.uint64), rg.view(np.uint64))


# ---------------------------------------------------------------- shapes ---
SHAPES = [(1, 1, 1), (63, 4, 4), (257, 20, 36), (1536, 256, 256), (1000, 304, 256),
          (20000, 16, 8)]
# fp16 pairs where K % 4 == 0
SWEEP = [(s, h2) for s in SHAPES for h2 in (False, True) if not (h2 and s[1] % 4)]


@pytest.mark.parametrize('shape,h2', SWEEP,
                         ids=['x'.join(str(v) for v in s) + ('-h2' if h else '-fp32')
                              for s, h in SWEEP])
def test_shape_sweep_to_bound(shape, h2):
  M, K, N = shape
  prob = random_problem(M, K, N, seed=M + K + N, h2=h2)
  if M == 20000:
    assert prob.ranges > 100                  # slabs and the closing pass
  if M == 1:
    assert prob.ranges == 1                   # written directly
  prob.check(*prob.run())


@pytest.mark.parametrize('h2', [False, True], ids=['fp32', 'h2'])
def test_padding_columns_are_never_read(h2):
  """lda > K and ldg > N with NaN in the padding; odd pads also take the fp32 rows off their
  16-byte alignment (the scalar loads)."""
  prob = random_problem(300, 20, 36, seed=9, h2=h2, pad=(4, 3) if h2 else (3, 5))
  S, g = prob.run()
  assert np.isfinite(S).all() and np.isfinite(g).all()
  prob.check(S, g)


def test_unaligned_fp32_operands():
  """A and G one float behind a 16-byte boundary, K and N odd: the scalar path."""
  M, K, N = 130, 7, 5
  prob = random_problem(M, K, N, seed=4)
  lib = _lib()
  a = torch.full((M * K + 1,), float('nan'), device='cuda')
  g_ = torch.full((M * N + 1,), float('nan'), device='cuda')
  a[1:] = prob.dA.view(torch.float32).reshape(-1)
  g_[1:] = prob.dG.reshape(-1)
  bS, S = _sent(K * N, torch.int64)
  bg, g = _sent(N, torch.int64)
  args = prob.args(S, g, A=_p(a[1:]), G=_p(g_[1:]))
  assert lib.epos_pointwise_wgrad_f32(ctypes.byref(args), _stream()) == 0
  torch.cuda.synchronize()
  prob.check(_check_sent(bS, K * N, 'S').view(np.float64).reshape(K, N),
             _check_sent(bg, N, 'g').view(np.float64))


# ------------------------------------------------- the device's own pairs ---
def test_fp16_pairs_written_by_the_depthwise_kernel():
  """A = what epos_depthwise3x3_f32 writes with y_h2 = 1, read by the gradient kernel with the
  same slots, gain and bias; the reference reconstructs A from the bytes the device wrote."""
  from epos_amd import _lib as binding
  lib = _lib()
  B, H, Wd, C, N = 2, 12, 16, 40, 24
  rng = np.random.RandomState(21)
  x = rng.randn(B, H, Wd, C).astype(np.float32)
  w9c = (0.5 * rng.randn(9, C)).astype(np.float32)
  bias = rng.randn(C).astype(np.float32)
  gain = float(np.abs(w9c.astype(np.float64)).sum(0).max())
  bias0 = float(np.abs(bias).max())
  slot = _slot(float(np.abs(x).max()), 9)
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
  prob = Problem(np.zeros((M, C), np.float32), G, h2=(slot, None, gain, bias0), raw=raw)
  # the pairs stand for the depthwise conv's outputs: relu'd, of the size of x * gain
  assert prob.A64.min() >= 0 and 0.1 < prob.A64.max() <= gain * np.abs(x).max() + bias0
  prob.dA = y                                                     # the device's own buffer
  prob.check(*prob.run())


# ---------------------------------------------------------------- closing ---
@pytest.mark.parametrize('K,N', [(256, 256), (20, 37), (1, 1)])
def test_batch_norm_closing(K, N):
  prob = random_problem(500, K, N, seed=K + N)
  S, g = prob.run()
  rS, rg, aS, ag = prob.reference()
  rng = np.random.RandomState(K)
  W = (0.3 * rng.randn(K, N)).astype(np.float32)
  bn = random_bn(N, seed=N)
  rc, dW, dgamma, dbeta = close(S, g, W, bn)
  assert rc == 0
  want = ref.close(rS, rg, W, *bn, eps=EPS)
  tol = ref.bounds_close(prob.M, rS, rg, aS, ag, W, *bn, eps=EPS)
  for got, w, t, what in zip((dW, dgamma, dbeta), want, tol, ('dW', 'dgamma', 'dbeta')):
    ok, worst = ref.within(got, w, t)
    print('%s K=%d N=%d: worst error / bound = %.3g' % (what, K, N, worst))
    assert ok, (what, worst)
  z = 1 % N                                                       # the gamma = 0 column
  assert not dW[:, z].view(np.uint32).any()                       # scale 0: +0.0
  if N > 1:
    assert dgamma[z] != 0 and np.abs(dW).max() > 0
  # from the device's own S and g the closing is a fixed sequence of fp64 operations: the
  # same bound without the summation term
  want = ref.close(S, g, W, *bn, eps=EPS)
  zero = np.zeros_like(aS), np.zeros_like(ag)
  tol = ref.bounds_close(prob.M, S, g, *zero, W, *bn, eps=EPS)
  for got, w, t in zip((dW, dgamma, dbeta), want, tol):
    assert ref.within(got, w, t)[0]


def test_closing_without_batch_norm():
  prob = random_problem(300, 20, 36, seed=2)
  S, g = prob.run()
  rc, dW, dgamma, db = close(S, g)
  assert rc == 0 and dgamma is None
  assert np.array_equal(dW.view(np.uint32), S.astype(np.float32).view(np.uint32))
  assert np.array_equal(db.view(np.uint32), g.astype(np.float32).view(np.uint32))


# ----------------------------------------------------------------- zeros ---
@pytest.mark.parametrize('h2', [False, True], ids=['fp32', 'h2'])
def test_zero_gradients_give_positive_zero_bytes(h2):
  """Rows with G = 0 add nothing; an all-zero G gives +0.0 bytes in S, g and, through a batch
  norm with negative gammas and means, in dW, dgamma and dbeta."""
  prob = random_problem(700, 20, 36, seed=6, h2=h2)
  S, g = prob.run()
  keep = np.arange(prob.M) % 3 != 1
  A2 = np.where(keep[:, None], prob.A64, 7.0).astype(np.float32)   # other A where G is zero
  G3 = np.where(keep[:, None], prob.G, 0.0).astype(np.float32)
  if not h2:
    p2 = Problem(A2, G3)
    S2, g2 = p2.run()
    p3 = Problem(prob.A64.astype(np.float32), G3)
    S3, g3 = p3.run()
    assert np.array_equal(S2.view(np.uint64), S3.view(np.uint64))   # zero rows add nothing
    assert np.array_equal(g2.view(np.uint64), g3.view(np.uint64))
  zero = Problem(-np.abs(prob.A64).astype(np.float32), np.zeros_like(prob.G), h2=prob.h2)
  S0, g0 = zero.run()
  assert not S0.view(np.uint64).any() and not g0.view(np.uint64).any()
  rng = np.random.RandomState(1)
  W = rng.randn(prob.K, prob.N).astype(np.float32)
  bn = (-1 - rng.rand(prob.N).astype(np.float32), -rng.rand(prob.N).astype(np.float32),
        np.ones(prob.N, np.float32))
  rc, dW, dgamma, dbeta = close(S0, g0, W, bn)
  assert rc == 0
  for out in (dW, dgamma, dbeta):
    assert not out.view(np.uint32).any()


# ----------------------------------------------------------- determinism ---
def test_two_runs_give_the_same_bytes():
  for h2 in (False, True):
    prob = random_problem(5000, 256, 256, seed=12, h2=h2)
    assert prob.ranges > 1
    S1, g1 = prob.run()
    S2, g2 = prob.run()
    assert np.array_equal(S1.view(np.uint64), S2.view(np.uint64))
    assert np.array_equal(g1.view(np.uint64), g2.view(np.uint64))


def test_non_finite_gradient_marks_its_column_only():
  M, K, N = 900, 24, 40
  prob = random_problem(M, K, N, seed=15)
  S, g = prob.run()
  c = 17
  G = prob.G.copy()
  G[401, c] = np.nan
  bad = Problem(prob.A64.astype(np.float32), G)
  Sb, gb = bad.run()
  others = np.arange(N) != c
  assert np.isnan(Sb[:, c]).all() and np.isnan(gb[c])
  assert np.array_equal(Sb[:, others].view(np.uint64), S[:, others].view(np.uint64))
  assert np.array_equal(gb[others].view(np.uint64), g[others].view(np.uint64))
  rng = np.random.RandomState(3)
  W = rng.randn(K, N).astype(np.float32)
  bn = random_bn(N, seed=5, zero_gamma=3)
  _, dW, dgamma, dbeta = close(S, g, W, bn)
  _, dWb, dgammab, dbetab = close(Sb, gb, W, bn)
  assert np.isnan(dWb[:, c]).all() and np.isnan(dgammab[c]) and np.isnan(dbetab[c])
  for a, b in ((dW, dWb), (dgamma, dgammab), (dbeta, dbetab)):
    assert np.array_equal(a[..., others].view(np.uint32), b[..., others].view(np.uint32))


# -------------------------------------------------------------- refusals ---
def test_refusals_leave_the_outputs_untouched():
  lib = _lib()
  h2 = random_problem(300, 20, 36, seed=1, h2=True, pad=(4, 0))
  f32 = random_problem(300, 20, 36, seed=1)
  assert f32.ranges > 1
  cases = [(f32, dict(A=None), b'null pointer'), (f32, dict(G=None), b'null pointer'),
           (f32, dict(S=None), b'null pointer'), (f32, dict(g=None), b'null pointer'),
           (f32, dict(workspace=None), b'the workspace must be given, 8-byte aligned'),
           (f32, dict(M=0), b'M, K and N must be positive'),
           (f32, dict(K=0), b'M, K and N must be positive'),
           (f32, dict(N=-1), b'M, K and N must be positive'),
           (f32, dict(lda=19), b'lda must be >= K'), (f32, dict(ldg=35), b'ldg must be >= N'),
           (h2, dict(a_amax=None), b'a pre-split A needs its absmax slot (a_amax)'),
           (h2, dict(lda=22), None), (h2, dict(K=18), None),
           (h2, dict(A=ctypes.c_void_p(h2.dA.data_ptr() + 4)), None)]
  for prob, over, msg in cases:
    bS, S = _sent(prob.K * prob.N, torch.int64)
    bg, g = _sent(prob.N, torch.int64)
    rc = lib.epos_pointwise_wgrad_f32(ctypes.byref(prob.args(S, g, **over)), _stream())
    assert rc == INVALID, over
    expect = msg or (b'a pre-split A needs K % 4 == 0, lda % 4 == 0 and 16-byte aligned rows')
    assert lib.epos_last_error() == b'epos_pointwise_wgrad_f32: ' + expect, over
    torch.cuda.synchronize()
    assert (bS.cpu().numpy() == SENT64).all() and (bg.cpu().numpy() == SENT64).all(), over
  assert lib.epos_pointwise_wgrad_f32(None, _stream()) == INVALID
  assert lib.epos_pointwise_wgrad_workspace_bytes(0, 4, 4) == INVALID
  # the closing entry
  S, g = np.ones((4, 6)), np.ones(6)
  W = np.ones((4, 6), np.float32)
  bn = random_bn(6, 0)
  null = ctypes.c_void_p(None)
  fake = ctypes.c_void_p(4096)
  for over in (dict(S=null), dict(g=null), dict(dW=null), dict(dbeta=null), dict(W=null),
               dict(mean=null), dict(var=null), dict(dgamma=null), dict(eps=-1.0),
               dict(eps=float('nan'))):
    assert close(S, g, W, bn, **over)[0] == INVALID, over
  assert close(S, g, W, bn, K=0)[0] == INVALID and close(S, g, W, bn, N=0)[0] == INVALID
  for over in (dict(mean=fake), dict(var=fake), dict(dgamma=fake)):
    assert close(S, g, **over)[0] == INVALID, over
  assert lib.epos_last_error().startswith(b'epos_pointwise_wgrad_close_f32: without gamma')


# ----------------------------------------------------------------- graph ---
def test_graph_capture_replays_to_the_same_bytes():
  lib = _lib()
  prob = random_problem(3000, 64, 72, seed=8, h2=True)
  assert prob.ranges > 1
  S1, g1 = prob.run()
  rng = np.random.RandomState(2)
  W = torch.from_numpy(rng.randn(prob.K, prob.N).astype(np.float32)).cuda()
  bn = [torch.from_numpy(v).cuda() for v in random_bn(prob.N, 4)]
  S = torch.zeros(prob.K * prob.N, dtype=torch.float64, device='cuda')
  g = torch.zeros(prob.N, dtype=torch.float64, device='cuda')
  outs = [torch.zeros(n, device='cuda') for n in (prob.K * prob.N, prob.N, prob.N)]

  def enqueue():
    s = _stream()
    assert lib.epos_pointwise_wgrad_f32(ctypes.byref(prob.args(S, g)), s) == 0
    assert lib.epos_pointwise_wgrad_close_f32(_p(S), _p(g), _p(W), prob.K, prob.N, _p(bn[0]),
                                              _p(bn[1]), _p(bn[2]), EPS, _p(outs[0]),
                                              _p(outs[1]), _p(outs[2]), s) == 0
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    enqueue()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  eager = [t.clone() for t in [S, g] + outs]
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    enqueue()
  for t in [S, g] + outs:
    t.fill_(-1.0)
  graph.replay()
  torch.cuda.synchronize()
  for a, b in zip(eager, [S, g] + outs):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
  assert np.array_equal(S.cpu().numpy().view(np.uint64).reshape(S1.shape), S1.view(np.uint64))
  assert np.array_equal(g.cpu().numpy().view(np.uint64), g1.view(np.uint64))
