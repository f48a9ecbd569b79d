"""epos_aspp_join_dgrad_f32 and epos_pool_broadcast_dgrad_f32 on the device (csrc/aspp_grad.hip),
through their wrappers and the C ABI, against tests/helpers/aspp_grad_ref.py -- the join bit for
bit, the broadcast's adjoint to its derived bound and bit for bit on integer data --, the cut of
K in pointwise_input_grad at ASPP's widths, and the existing depthwise kernels at rates that
leave the image. Outputs are pre-filled with a sentinel: every element must be written and
nothing around them touched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import aspp_grad_ref as aref                           # noqa: E402
from tests.helpers import decoder_backward_ref as ref                     # noqa: E402
from tests.helpers import pointwise_wgrad_ref as wref                     # noqa: E402

pytestmark = pytest.mark.gpu

SENT32 = 0x7FA55A5A                        # a NaN no kernel produces
GUARD = 64                                 # sentinel words behind the last row
EPS = 1e-5


def bits(t):
  return t.detach().cpu().contiguous().numpy().view(np.uint32)


def wide(a, ld):
  """a [..., C] on the device as a slice of a NaN-filled buffer with rows of ld floats."""
  a = np.ascontiguousarray(a, np.float32)
  own = torch.full(a.shape[:-1] + (ld,), float('nan'), device='cuda')
  own[..., :a.shape[-1]] = torch.from_numpy(a).cuda()
  return own[..., :a.shape[-1]]


def sentinel_out(shape, ld):
  """(the owning int32 buffer, its [..., C] float view): rows of ld words, GUARD words behind."""
  rows = int(np.prod(shape[:-1]))
  own = torch.full((rows * ld + GUARD,), SENT32, dtype=torch.int32, device='cuda')
  return own, own[:rows * ld].view(torch.float32).view(shape[:-1] + (ld,))[..., :shape[-1]]


def written(own, shape, ld, what):
  """[..., C] uint32 of a sentinel_out buffer: all written, padding and guard untouched."""
  raw = own.cpu().numpy().view(np.uint32)
  rows = int(np.prod(shape[:-1]))
  body = raw[:rows * ld].reshape(rows, ld)
  assert (raw[rows * ld:] == SENT32).all(), '%s: written behind the last row' % what
  assert (body[:, shape[-1]:] == SENT32).all(), '%s: padding columns written' % what
  assert not (body[:, :shape[-1]] == SENT32).any(), '%s: elements not written' % what
  return np.ascontiguousarray(body[:, :shape[-1]]).reshape(shape)


# ================================================================= join ===
class JoinCase(object):
  """Host data of one shape: four depthwise terms at `rates` (cycled), two plain terms, a pool
  and a mask with -0.0, +0.0 and a NaN in it; lds = (input ld, output ld)."""

  def __init__(self, B, H, W, C, rates, lds=None, seed=0):
    rng = np.random.RandomState(seed)
    self.shape = (B, H, W, C)
    self.rates = tuple(rates[i % len(rates)] for i in range(4))
    self.n_rates = len(rates)
    self.lds = lds or (C, C)
    f32 = np.float32
    self.D = [rng.randn(B, H, W, C).astype(f32) for _ in range(4)]
    self.w = [(0.5 * rng.randn(9, C)).astype(f32) for _ in range(4)]
    self.E = [rng.randn(B, H, W, C).astype(f32) for _ in range(2)]
    self.pool = rng.randn(B, C).astype(f32)
    Y = rng.randn(B, H, W, C).astype(f32)
    flat = Y.reshape(-1)
    flat[0::7] = 0.0
    flat[1::7] = -0.0
    flat[2::31] = np.nan
    self.Y = Y
    ld = self.lds[0]
    self.dD = [wide(d, ld) for d in self.D]
    self.dw = [torch.from_numpy(w).cuda() for w in self.w]
    self.dE = [wide(e, ld) for e in self.E]
    self.dpool = wide(self.pool, ld)
    self.dY = wide(Y, ld)

  def run(self, n_dw, n_plain, div, mask, partition='shipped'):
    from epos_amd import decoder_train as DT
    own, out = sentinel_out(self.shape, self.lds[1])
    got = DT.aspp_join_grad(
        depthwise=[(self.dD[i], self.dw[i], self.rates[i]) for i in range(n_dw)],
        plain=self.dE[:n_plain], pooled=(self.dpool, div) if div else None,
        relu_of=self.dY if mask else None, out=out, partition=partition)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return written(own, self.shape, self.lds[1], 'dX %s' % (self.shape,))

  def want(self, n_dw, n_plain, div, mask):
    return aref.aspp_join_ref(
        self.shape, [(self.D[i], self.w[i], self.rates[i]) for i in range(n_dw)],
        self.E[:n_plain], (self.pool, div) if div else None, self.Y if mask else None)


JOIN_SHAPES = {
    'smallest': (1, 1, 1, 4, (1,), None),
    'every_tap_live': (2, 5, 7, 8, (1, 2, 3), None),
    'taps_in_the_padding': (1, 12, 16, 64, (12, 24, 36), None),
    'partial_block_padded_rows': (2, 9, 11, 132, (2, 5), (136, 144)),
    'real_width': (1, 3, 40, 2048, (6,), None),
}


@pytest.mark.parametrize('name', sorted(JOIN_SHAPES))
def test_join_is_bit_equal_to_its_restatement(name):
  B, H, W, C, rates, lds = JOIN_SHAPES[name]
  case = JoinCase(B, H, W, C, rates, lds, seed=len(name))
  n = case.n_rates
  # (n_dw, n_plain, pool_div or None, mask): with and without the mask, 0 / 1 / 2 plain terms,
  # no pool / H W / 1, n_dw = 0 and 4 once each
  configs = [(n, 1, H * W, True), (n, 0, None, False), (n, 2, 1, True), (0, 2, H * W, True),
             (4, 1, None, False), (0, 0, 1, False), (n, 0, H * W, True)]
  for cfg in configs:
    got, want = case.run(*cfg), case.want(*cfg)
    same = np.array_equal(got, want.view(np.uint32))
    print('join %s %s n_dw=%d n_plain=%d div=%s mask=%s: %s' % (
        name, case.shape, cfg[0], cfg[1], cfg[2], cfg[3], 'bit-equal' if same else 'DIFFERS'))
    assert same, (name, cfg, int((got != want.view(np.uint32)).sum()))
    if cfg[3]:
      with np.errstate(invalid='ignore'):
        assert not got[case.Y <= 0].any()                   # the BYTES of +0.0
  # the partition decides who computes an element, never its value
  first = case.run(*configs[0])
  for partition in ('pixel', 'slice32', 'slice64', 'slice32x2', 'slice32x4'):
    assert np.array_equal(case.run(*configs[0], partition=partition), first), partition


def test_masked_elements_are_plus_zero_where_the_sum_is_negative_or_minus_zero():
  from epos_amd import decoder_train as DT
  shape = (1, 2, 2, 4)
  D = np.full(shape, -1e-40, np.float32)                   # w * d = -1e-80: rounds to -0.0
  w = np.zeros((9, 4), np.float32)
  w[4] = 1e-40
  E = np.full(shape, -3.0, np.float32)
  Y = np.float32([1.0, 0.0, -0.0, -2.0] * 4).reshape(shape)
  dD, dw_, dE, dY = (torch.from_numpy(a).cuda() for a in (D, w, E, Y))
  open_ = bits(DT.aspp_join_grad(depthwise=[(dD, dw_, 1)]))
  assert (open_ == 0x80000000).all()                       # -0.0 without a mask
  shut = bits(DT.aspp_join_grad(depthwise=[(dD, dw_, 1)], relu_of=dY))
  assert shut[0, 0, 0].tolist() == [0x80000000, 0, 0, 0]
  neg = bits(DT.aspp_join_grad(plain=[dE], relu_of=dY)).view(np.float32)
  assert neg[0, 0, 0].tolist() == [-3.0, 0.0, 0.0, 0.0] and not bits(
      DT.aspp_join_grad(plain=[dE], relu_of=dY))[..., 1:].any()


def test_one_depthwise_term_alone_is_depthwise_input_grad():
  from epos_amd import decoder_train as DT
  case = JoinCase(2, 9, 11, 132, (2, 5), (136, 144), seed=3)
  for i, mask in ((0, True), (1, False)):
    y = case.dY if mask else None
    a = DT.aspp_join_grad(depthwise=[(case.dD[i], case.dw[i], case.rates[i])], relu_of=y)
    b = DT.depthwise_input_grad(case.dD[i], case.dw[i], rate=case.rates[i], relu_of=y)
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(a), ref.depthwise_dgrad(case.D[i], case.w[i], case.rates[i],
                                                       Y=case.Y if mask else None).view(np.uint32))


def join_of(case, sl=slice(None)):
  from epos_amd import decoder_train as DT
  return DT.aspp_join_grad(
      depthwise=[(case.dD[i][sl], case.dw[i], case.rates[i]) for i in range(3)],
      plain=[case.dE[0][sl]], pooled=(case.dpool[sl], 35), relu_of=case.dY[sl])


def test_join_image_position_repeat_side_stream_and_graph_replay():
  from epos_amd import decoder_train as DT
  case = JoinCase(3, 5, 7, 8, (1, 2, 3), seed=11)
  batch = join_of(case)
  torch.cuda.synchronize()
  want = case.want(3, 1, 35, True).view(np.uint32)
  assert np.array_equal(bits(batch), want)
  for b in range(3):                                       # an image alone
    assert np.array_equal(bits(join_of(case, slice(b, b + 1))), want[b:b + 1]), b
  assert np.array_equal(bits(join_of(case)), want)         # the same bytes twice
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    on_side = join_of(case)
  side.synchronize()
  assert np.array_equal(bits(on_side), want)
  # a captured graph's replay: one chain of launches
  out = torch.empty((3, 5, 7, 8), device='cuda')
  terms = [(case.dD[i], case.dw[i], case.rates[i]) for i in range(3)]
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    DT.aspp_join_grad(depthwise=terms, plain=[case.dE[0]], pooled=(case.dpool, 35),
                      relu_of=case.dY, out=out)
  for _ in range(2):
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), want)


def test_join_refusals_leave_the_sentinels():
  from epos_amd import decoder_train as DT
  from epos_amd._lib import EposError
  case = JoinCase(1, 3, 4, 8, (1,), seed=2)
  own, out = sentinel_out(case.shape, 8)
  with pytest.raises(EposError, match='rate must be >= 1'):
    DT.aspp_join_grad(depthwise=[(case.dD[0], case.dw[0], 0)], out=out)
  with pytest.raises(EposError, match='pool_div must be >= 1'):
    DT.aspp_join_grad(pooled=(case.dpool, 0), out=out)
  with pytest.raises(EposError, match='dX may not start at an input'):
    DT.aspp_join_grad(plain=[case.dE[0]], out=case.dE[0])
  with pytest.raises(ValueError, match='at least one term'):
    DT.aspp_join_grad(relu_of=case.dY, out=out)
  with pytest.raises(ValueError, match='at most 4 depthwise'):
    DT.aspp_join_grad(depthwise=[(case.dD[0], case.dw[0], 1)] * 5, out=out)
  torch.cuda.synchronize()
  assert (own.cpu().numpy().view(np.uint32) == SENT32).all()


# ================================================= the broadcast's adjoint ===
POOL_SHAPES = [(3, 1, 4, 4), (2, 35, 8, 8), (2, 63, 12, 12), (2, 64, 12, 12), (2, 65, 12, 12),
               (2, 192, 256, 1280), (1, 4800, 256, 256)]


@pytest.mark.parametrize('B,P,C,ld', POOL_SHAPES)
def test_pool_broadcast_grad(B, P, C, ld):
  """Bit-equal on integers (every order of an exact sum gives the same bits), within the bound
  on random data; sentinels; an image alone; the same bytes twice."""
  from epos_amd import decoder_train as DT
  lib = DT._lib.load()
  count = -(-P // lib.epos_pool_broadcast_dgrad_range_pixels(B, P, C))
  assert lib.epos_pool_broadcast_dgrad_workspace_bytes(B, P, C) == (
      0 if count == 1 else 8 * count * B * C)
  rng = np.random.RandomState(P + C)
  ints = rng.randint(-2000, 2000, size=(B, P, C)).astype(np.float32)
  rand = (rng.randn(B, P, C) * np.exp(3 * rng.randn(B, P, C))).astype(np.float32)
  for data, exact in ((ints, True), (rand, False)):
    d = wide(data, ld)                                     # a column slice of a wider buffer
    own, out = sentinel_out((B, C), C + 4)
    got = DT.pool_broadcast_grad(d, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    g = written(own, (B, C), C + 4, 'g').view(np.float32)
    want, bound = aref.pool_broadcast_ref(data)
    if exact:
      assert np.array_equal(g, want.astype(np.float32))
    ok, worst = wref.within(g, want, bound)
    print('pool B=%d P=%d C=%d ld=%d (%d ranges) %s: worst error / bound = %.3g' % (
        B, P, C, ld, count, 'integers' if exact else 'random', worst))
    assert ok, worst
    again = DT.pool_broadcast_grad(d.view(B, P, 1, C) if P > 1 else d)   # [B,H,W,C] too
    assert np.array_equal(bits(again), g.view(np.uint32))
    for b in range(B):                                     # an image alone
      assert np.array_equal(bits(DT.pool_broadcast_grad(d[b:b + 1])), g.view(np.uint32)[b:b + 1])


def test_pool_broadcast_grad_on_a_side_stream_and_in_a_graph():
  from epos_amd import decoder_train as DT
  B, P, C = 2, 192, 256
  d = torch.randn(B, P, C, device='cuda')
  eager = DT.pool_broadcast_grad(d)
  ws = torch.empty(DT.pool_workspace_bytes(B, P, C) // 8, dtype=torch.float64, device='cuda')
  out = torch.empty(B, C, device='cuda')
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    on_side = DT.pool_broadcast_grad(d, workspace=ws)
  side.synchronize()
  assert np.array_equal(bits(on_side), bits(eager))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    DT.pool_broadcast_grad(d, out=out, workspace=ws)
  for _ in range(2):
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), bits(eager))
  with pytest.raises(ValueError, match='workspace'):
    DT.pool_broadcast_grad(d, workspace=ws[:8])


# =================================== pointwise_input_grad beyond K = 1024 ===
@pytest.fixture(scope='module')
def wide_dgrad():
  """G [40,256], folded-layer inputs for K = 2048 (K = 1280 reads its first rows) and a mask."""
  rng = np.random.RandomState(5)
  M, N, K = 40, 256, 2048
  G = rng.randn(M, N).astype(np.float32)
  Wm = (0.1 * rng.randn(K, N)).astype(np.float32)
  gamma = (0.5 + rng.rand(N)).astype(np.float32)
  var = (0.2 + rng.rand(N)).astype(np.float32)
  A = np.maximum(rng.randn(M, K), 0).astype(np.float32)    # behind a ReLU: about half shut
  return G, Wm, gamma, var, A


def count_calls(monkeypatch):
  """Counts the ABI calls of the input gradient through a wrapper around the bound function."""
  from epos_amd import _lib
  lib = _lib.load()
  calls = {'dgrad': [], 'bytes': []}
  real, real_bytes = lib.epos_pointwise_dgrad_f32, lib.epos_pointwise_dgrad_workspace_bytes

  def dgrad(args, stream):
    calls['dgrad'].append(int(args._obj.K))
    return real(args, stream)

  def nbytes(K, N):
    calls['bytes'].append((K, N))
    return real_bytes(K, N)
  monkeypatch.setattr(lib, 'epos_pointwise_dgrad_f32', dgrad)
  monkeypatch.setattr(lib, 'epos_pointwise_dgrad_workspace_bytes', nbytes)
  return calls


@pytest.mark.parametrize('K', [1280, 2048])
@pytest.mark.parametrize('mask', ['f32', 'h2', None])
def test_pointwise_input_grad_cuts_a_wide_k(wide_dgrad, K, mask, monkeypatch):
  from epos_amd import _call as Cc, _lib, decoder_train as DT
  G, Wm, gamma, var, A = wide_dgrad
  Wm, A = Wm[:K], A[:, :K]
  M, N = G.shape
  dG, dW = torch.from_numpy(G).cuda(), torch.from_numpy(np.ascontiguousarray(Wm)).cuda()
  bn = (torch.from_numpy(gamma).cuda(), torch.from_numpy(var).cuda())
  dmask, values = None, None
  if mask == 'f32':
    dmask, values = torch.from_numpy(np.ascontiguousarray(A)).cuda(), A
  elif mask == 'h2':
    raw = wref.h2_split(np.ascontiguousarray(A), 2.0 ** 10)
    dmask, values = torch.from_numpy(raw).cuda(), ref.pair_values(raw, K)
  calls = count_calls(monkeypatch)
  own, out = sentinel_out((M, K), K + 8)
  DT.pointwise_input_grad(dG, dW, bn=bn, eps=EPS, relu_of=dmask, relu_of_h2=mask == 'h2',
                          out=out)
  torch.cuda.synchronize()
  assert calls['dgrad'] == [k1 - k0 for k0, k1 in DT.k_blocks(K)] and len(calls['dgrad']) == 2
  assert calls['bytes'] == [(1024, N)]                     # a workspace for one block
  got = written(own, (M, K), K + 8, 'D')
  Wf = ref.fold(Wm, gamma, var, EPS)
  want, absum = ref.pointwise_dgrad(G, Wf, values)
  ok, worst = wref.within(got.view(np.float32), want, ref.bound_pointwise_dgrad(N, want, absum))
  print('D M=%d K=%d N=%d mask=%s: worst error / bound = %.3g' % (M, K, N, mask, worst))
  assert ok and np.abs(got.view(np.float32)).max() > 0, worst
  if values is not None:
    assert (values <= 0).any() and not got[values <= 0].any()
  # the entry by hand in blocks of 640: the same bytes
  lib = _lib.load()
  hand = torch.full((M, K), float('nan'), device='cuda')
  ws = torch.empty(lib.epos_pointwise_dgrad_workspace_bytes(640, N) // 8, dtype=torch.float64,
                   device='cuda')
  for k0 in range(0, K, 640):
    k1 = min(k0 + 640, K)
    args = _lib.PointwiseDgradArgs(
        G=Cc.ptr(dG), ldg=N, W=Cc.ptr(dW, k0 * N), gamma=Cc.ptr(bn[0]),
        moving_variance=Cc.ptr(bn[1]), eps=EPS, mask=Cc.ptr(dmask, k0), ldm=K,
        mask_h2=int(mask == 'h2'), M=M, K=k1 - k0, N=N, D=Cc.ptr(hand, k0), ldd=K,
        workspace=Cc.ptr(ws))
    _lib.check(lib.epos_pointwise_dgrad_f32(ctypes.byref(args), Cc.stream_handle(dG.device)[1]),
               'epos_pointwise_dgrad_f32')
  torch.cuda.synchronize()
  assert np.array_equal(bits(hand), got)


def test_a_narrow_k_makes_the_calls_it_made(wide_dgrad, monkeypatch):
  from epos_amd import decoder_train as DT
  from epos_amd._lib import EposError
  G, Wm, gamma, var, A = wide_dgrad
  dG, dW = torch.from_numpy(G).cuda(), torch.from_numpy(np.ascontiguousarray(Wm[:256])).cuda()
  calls = count_calls(monkeypatch)
  DT.pointwise_input_grad(dG, dW)
  torch.cuda.synchronize()
  assert calls['dgrad'] == [256] and calls['bytes'] == [(256, 256)]
  wideN = torch.zeros(8, 1028, device='cuda')              # N > 1024 stays refused
  with pytest.raises(EposError, match='K and N must be in 1..1024'):
    DT.pointwise_input_grad(wideN, torch.zeros(8, 1028, device='cuda'))


# ========================= the depthwise kernels at rates that leave the image ===
@pytest.mark.parametrize('rate', [7, 9])
def test_depthwise_kernels_at_a_rate_beyond_the_image(rate):
  """(1, 5, 7, 8): rate 7 >= H and >= W, rate 9 > both -- only the centre tap is ever inside."""
  from epos_amd import decoder_train as DT
  rng = np.random.RandomState(rate)
  B, H, W, C = 1, 5, 7, 8
  X, D = (rng.randn(B, H, W, C).astype(np.float32) for _ in range(2))
  w = (0.5 * rng.randn(3, 3, C, 1)).astype(np.float32)
  gamma, mean = (rng.randn(C).astype(np.float32) for _ in range(2))
  var = (0.2 + rng.rand(C)).astype(np.float32)
  w9c = (0.5 * rng.randn(9, C)).astype(np.float32)
  dX, dD, dw_, dw9 = (torch.from_numpy(a).cuda() for a in (X, D, w, w9c))
  bn = tuple(torch.from_numpy(a).cuda() for a in (gamma, mean, var))
  got = DT.depthwise_input_grad(dD, dw9, rate=rate, relu_of=dX)
  assert np.array_equal(bits(got), ref.depthwise_dgrad(D, w9c, rate, Y=X).view(np.uint32))
  centre = np.where(X <= 0, np.float32(0), (w9c[4].astype(np.float64) * D).astype(np.float32))
  assert np.array_equal(bits(got), centre.view(np.uint32))
  grads = DT.depthwise_weight_grads(dX, dD, dw_, bn, EPS, rate=rate)
  T, t, aT, at = ref.depthwise_wgrad(X, D, rate)
  assert not T[:4].any() and not T[5:].any() and T[4].any()
  want = wref.close(T, t, w.reshape(9, C), gamma, mean, var, EPS)
  tol = wref.bounds_close(B * H * W, T, t, aT, at, w.reshape(9, C), gamma, mean, var, EPS)
  for short, wv, tv in zip(('depthwise_weights', 'BatchNorm/gamma', 'BatchNorm/beta'), want, tol):
    ok, worst = wref.within(grads[short].cpu().numpy().reshape(wv.shape), wv, tv)
    print('depthwise rate %d %s: worst error / bound = %.3g' % (rate, short, worst))
    assert ok, (short, worst)
