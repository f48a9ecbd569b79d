"""The two product kernels behind epos_pointwise_conv_grouped_f32 that are not the fp16-pair GEMM
-- pointwise_gemv_f32 (one problem, M <= 8, sub == 1: csrc/pointwise_gemm.hip) and
pointwise_gemm_split_f32 (bf16 x 6: csrc/pointwise_gemm_split.hip) -- in every launch regime of
tests/helpers/gemm_fallback_cases.py, through the C ABI of the PRODUCT library, and the routing
between them. Every case asserts
 (a) accuracy against fp64. GEMV: |got - exact| <= (n + 18) 2^-24 1.01 mag with n = 4 ceil(K / 64)
     (derived: helpers' gemv_bound), and bit equality with the numpy restatement of the kernel's
     summation order on every element the restatement does not flag. Split: |got - exact| <=
     H2_MAX_REL_ERR mag. Exact-integer inputs: bit-equal to the integer product in both;
 (b) no stray writes and no NaN in C: C lies in a sentinel-filled buffer with guard rows, A's
     padding columns, the rows behind its last one and the rows a stride-2 gather skips are
     NaN, and so is everything around R and the bias;
 (c) two runs give the same bytes; a group gives the bytes of its problems launched one by one;
     c_amax == max |C| exactly, also for a group writing column slices of one buffer.
The routing table of the issue is asserted row by row (test_routing_*), refusals leave every
output untouched, and one case per kernel runs on a non-default stream, in a captured graph and
between launches of another instantiation. Inputs and expectations are computed once per
problem (helpers' lru_cache)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import gemm_fallback_cases as fc

pytestmark = pytest.mark.gpu

CASES = fc.by_name(fc.ALL_CASES)
SENT = np.int32(fc.SENTINEL_BITS)


@pytest.fixture(scope='module')
def lib():
  from epos_amd import _lib
  assert torch.cuda.is_available(), 'GPU tests need a HIP device'
  return _lib.load()


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(words):
  """A uint32 / int32 / float32 host array on the device, bit for bit, as int32."""
  return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).cuda()


def _sentinels(*shape):
  return torch.full(shape, fc.SENTINEL_BITS, dtype=torch.int32, device='cuda')


def _pack(lib, w, which):
  k, n = w.shape
  fn = {'plain': lib.epos_pack_pointwise_weights, 'split': lib.epos_pack_pointwise_weights_split,
        'h2': lib.epos_pack_pointwise_weights_h2}[which]
  w = np.ascontiguousarray(w, np.float32)
  src = w.ctypes.data_as(ctypes.c_void_p)
  total = fn(src, k, n, None)
  assert total > 0, which
  dst = np.empty(total, np.float32 if which == 'plain' else np.uint8)
  fn(src, k, n, dst.ctypes.data_as(ctypes.c_void_p))
  return torch.from_numpy(dst).cuda()


def _slot(value=None):
  from epos_amd import _lib
  s = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device='cuda')
  if value is not None:
    s[37] = int(np.array([value], np.float32).view(np.int32)[0])
  return s


def _slot_value(slot):
  return float(slot.cpu().numpy().view(np.float32).max())


class Problem(object):
  """One problem's inputs on the device. has: which of 'Ws', 'Wh', 'a_amax', 'a_presplit' the
  call brings besides Wp."""

  def __init__(self, lib, p, inp, has):
    self.p, self.inp, self.has = p, inp, frozenset(has)
    self.A = _dev(fc.a_buffer(p, inp))
    self.Wp = _pack(lib, inp.w, 'plain')
    self.Ws = _pack(lib, inp.w, 'split') if 'Ws' in has else None
    self.Wh = _pack(lib, inp.w, 'h2') if 'Wh' in has else None
    finite = np.abs(inp.a[np.isfinite(inp.a)])
    self.slot = _slot(finite.max()) if 'a_amax' in has else None
    self.bias = _dev(fc.bias_buffer(p, inp.bias)) if p.bias else None
    self.R = _dev(fc.r_buffer(p, inp.r)) if p.res else None
    assert self.A.data_ptr() % 16 == 0


class Group(object):
  """Problems on the device, their launches and their outputs on the host."""

  def __init__(self, lib, case, has=None, inputs=None):
    self.lib, self.case = lib, case
    if has is None:
      has = ('Ws',) if case.kernel == 'split' else (('Ws', 'Wh', 'a_amax') if case.extra else ())
    if inputs is None:
      inputs = [fc.inputs(case.name, i) for i in range(len(case.problems))]
    self.inputs = inputs
    self.problems = [Problem(lib, p, inp, has) for p, inp in zip(case.problems, inputs)]
    self.layout, self.places = fc.layout(case), fc.places(case)

  def buffers(self):
    """Fresh outputs: (C buffers, c_amax slot per problem)."""
    bufs = [_sentinels(b.floats) for b in self.layout]
    assert all(b.data_ptr() % 512 == 0 for b in bufs)
    shared_slot = _slot() if self.case.shared else None
    amax = [(shared_slot if self.case.shared else _slot()) if d.p.c_amax else None
            for d in self.problems]
    return bufs, amax

  def args(self, out, wp_only=False):
    from epos_amd import _lib
    bufs, amax = out
    arr = (_lib.PointwiseArgs * len(self.problems))()
    for i, (d, (bi, off, ldc)) in enumerate(zip(self.problems, self.places)):
      p = d.p
      ho, wo = fc.out_hw(p)
      extra = not wp_only
      arr[i] = _lib.PointwiseArgs(
          A=d.A.data_ptr(), lda=p.lda, Wp=d.Wp.data_ptr(),
          bias=d.bias.data_ptr() + 4 * fc.BIAS_GUARD if d.bias is not None else None,
          R=d.R.data_ptr() + 4 * fc.R_GUARD_ROWS * p.ldr if d.R is not None else None, ldr=p.ldr,
          C=bufs[bi].data_ptr() + 4 * off, ldc=ldc, M=p.m, N=p.n, K=p.k, relu=p.relu,
          relu_in=p.relu_in, sub=p.sub, Ho=ho, Wo=wo, Hi=p.hi, Wi=p.wi,
          Ws=d.Ws.data_ptr() if extra and d.Ws is not None else None,
          Wh=d.Wh.data_ptr() if extra and d.Wh is not None else None,
          a_amax=d.slot.data_ptr() if extra and d.slot is not None else None,
          a_presplit=1 if 'a_presplit' in d.has else 0,
          c_amax=amax[i].data_ptr() if amax[i] is not None else None)
    return arr

  def call(self, out, one_by_one=False, wp_only=False):
    """Enqueues the case on the current stream; returns (return codes, what must stay alive)."""
    arr = self.args(out, wp_only)
    if one_by_one:
      rcs = [self.lib.epos_pointwise_conv_f32(ctypes.byref(arr[i]), _stream())
             for i in range(len(self.problems))]
    else:
      rcs = [self.lib.epos_pointwise_conv_grouped_f32(arr, len(self.problems), _stream())]
    return rcs, arr

  def launch(self, out, **kw):
    from epos_amd import _lib
    rcs, arr = self.call(out, **kw)
    for rc in rcs:
      _lib.check(rc, self.case.name, lib=self.lib)
    return arr

  @staticmethod
  def fetch(out):
    bufs, amax = out
    return ([b.cpu().numpy() for b in bufs],
            [_slot_value(a) if a is not None else None for a in amax])

  def run(self, **kw):
    out = self.buffers()
    keep = self.launch(out, **kw)
    torch.cuda.synchronize()
    del keep
    return self.fetch(out)

  def values(self, bufs, i):
    bi, off, ldc = self.places[i]
    p = self.case.problems[i]
    idx = off + np.arange(p.m)[:, None] * ldc + np.arange(p.n)[None, :]
    return bufs[bi][idx].view(np.float32)


def _same(a, b, what):
  """Equal bytes of two fetched results (C buffers, c_amax values)."""
  for x, y in zip(a[0], b[0]):
    diff = np.flatnonzero(x != y)
    assert diff.size == 0, '%s: %d words of C differ (first at %d)' % (what, diff.size, diff[0])
  assert a[1] == b[1], (what, a[1], b[1])


def _check_writes(case, bufs):
  """(b): everything the case must write is written, every other word keeps the sentinel."""
  for bi, out in enumerate(bufs):
    mask = fc.written_mask(case, bi)
    left = int((out[mask] == SENT).sum())
    assert left == 0, '%s: %d elements of buffer %d unwritten' % (case.name, left, bi)
    broken = np.flatnonzero(out[~mask] != SENT)
    assert broken.size == 0, '%s: %d words written outside [M) x [c_off, c_off + N) of buffer ' \
        '%d (first at index %d of the outside)' % (case.name, broken.size, bi, broken[0])


def _ratio(err, bound):
  live = bound > 0
  assert (err[~live] == 0).all()
  return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _fp32_mfma_ratio(p, inp):
  """The yardstick of the split bar: the fp32-MFMA kernel of the TEST build on the same inputs,
  worst |got - exact| / (H2_MAX_REL_ERR mag)."""
  from epos_amd import _lib
  ref = _lib.load_ref()
  case = fc.Case('yardstick', 'split', [p], ['vec'])
  g = Group(ref, case, has=(), inputs=[inp])
  bufs, _ = g.run()
  _check_writes(case, bufs)
  exact, mag = fc.expectation(p, inp)
  got = g.values(bufs, 0)
  assert np.isfinite(got).all()
  return _ratio(np.abs(got.astype(np.float64) - exact), fc.H2_MAX_REL_ERR * mag)


def _check_split(g, bufs):
  """(a) for the split kernel; returns the worst error / bound."""
  case, worst = g.case, 0.0
  for i, p in enumerate(case.problems):
    exact, mag = fc.expectation(p, g.inputs[i])
    got = g.values(bufs, i)
    assert np.isfinite(got).all(), '%s: problem %d has non-finite values' % (case.name, i)
    if case.values == 'integers':
      assert np.array_equal(got.astype(np.float64), exact), \
          '%s: problem %d is not the integer product' % (case.name, i)
      continue
    err = np.abs(got.astype(np.float64) - exact)
    ratio = _ratio(err, fc.H2_MAX_REL_ERR * mag)
    worst = max(worst, ratio)
    print('%s problem %d (%d x %d x %d): worst error / (H2_MAX_REL_ERR * mag) = %.4f' % (
        case.name, i, p.m, p.n, p.k, ratio))
    if ratio > 1.0:
      yard = _fp32_mfma_ratio(p, g.inputs[i])
      assert False, '%s problem %d: %.4f of the bar; the fp32-MFMA kernel on the same inputs: ' \
          '%.4f (above 1 / 1.5: the inputs are at fault, below: the kernel)' % (
              case.name, i, ratio, yard)
  return worst


def _check_gemv(g, bufs):
  """(a) for the GEMV; returns the worst error / derived bound."""
  case = g.case
  p, = case.problems
  inp = g.inputs[0]
  exact, mag = fc.expectation(p, inp)
  want, flagged = fc.gemv_restate(p, inp)
  got = g.values(bufs, 0)
  bad = ~np.isfinite(inp.a).all(axis=1)
  assert bad.any() == (case.values == 'nan_row')
  assert not np.isfinite(got[bad]).any(), '%s: a row fed by NaN and Inf came out finite' % case.name
  assert np.isfinite(got[~bad]).all(), '%s: non-finite values outside the bad row' % case.name
  frac = float(flagged.mean())
  assert frac < fc.FLAG_CAP or not flagged.any(), (case.name, frac)
  keep = ~flagged & ~bad[:, None]
  diff = np.flatnonzero(got.view(np.uint32)[keep] != want.view(np.uint32)[keep])
  assert diff.size == 0, '%s: %d of %d unflagged elements differ from the restated order' % (
      case.name, diff.size, keep.sum())
  if case.values == 'integers':
    assert np.array_equal(got.astype(np.float64), exact), case.name
    return 0.0
  if case.values == 'negative':                  # relu_in leaves nothing of A: bias (+ R) exactly
    assert np.array_equal(got, (np.float32(0) + inp.bias) + inp.r), case.name
  err = np.abs(got[~bad].astype(np.float64) - exact[~bad])
  ratio = _ratio(err, fc.gemv_bound(p, mag[~bad]))
  print('%s (%d x %d x %d): worst error / derived bound = %.4f, %d of %d elements flagged' % (
      case.name, p.m, p.n, p.k, ratio, flagged.sum(), flagged.size))
  assert ratio <= 1.0, (case.name, ratio)
  return ratio


def _check_amax(g, res):
  """c_amax == max |C| over what the launch wrote -- a shared slot over every slice."""
  case = g.case
  bufs, amax = res
  tops = [float(np.abs(g.values(bufs, i)).max()) for i in range(len(case.problems))]
  for i, p in enumerate(case.problems):
    if p.c_amax:
      want = max(t for t, q in zip(tops, case.problems) if q.c_amax) if case.shared else tops[i]
      assert amax[i] == want and want > 0, (case.name, i, amax[i], want)


# ------------------------------------------------------------------------------- regimes ---
@pytest.mark.parametrize('name', [c.name for c in fc.GEMV_CASES])
def test_gemv_regime(lib, name):
  case = CASES[name]
  g = Group(lib, case)
  res = g.run()
  _check_writes(case, res[0])
  worst = _check_gemv(g, res[0])
  print('%s: worst error / bound %.4f' % (name, worst))
  _same(res, g.run(), name + ': second run')
  if case.extra:                # Wh, Ws and a bound for A change nothing
    _same(res, g.run(wp_only=True), name + ': Wp only')


@pytest.mark.parametrize('name', [c.name for c in fc.SPLIT_CASES])
def test_split_regime(lib, name):
  case = CASES[name]
  g = Group(lib, case)
  res = g.run()
  _check_writes(case, res[0])
  worst = _check_split(g, res[0])
  _check_amax(g, res)
  print('%s: worst error / bound %.4f' % (name, worst))
  _same(res, g.run(), name + ': second run')
  if len(case.problems) > 1:
    one = g.run(one_by_one=True)
    _same(res, one, name + ': problem by problem')
    _check_writes(case, one[0])


def test_split_is_no_worse_than_the_fp32_mfma_yardstick(lib):
  """The claim the split kernel rests on (test_pointwise_gemm_split_accuracy asserts it on three
  large single problems): its worst error is not above 1.5 times that of the fp32-MFMA kernel of
  the test build on the same inputs. Here on tables' inputs with a residual, a long and a
  one-step K and a banded N -- the larger cases of the 64-row table, where a maximum over the
  elements means something."""
  for name in ('k128_res', 'k728_long', 'band_64'):
    case = CASES[name]
    p, inp = case.problems[0], fc.inputs(name, 0)
    g = Group(lib, case)
    bufs, _ = g.run()
    exact, mag = fc.expectation(p, inp)
    mine = _ratio(np.abs(g.values(bufs, 0).astype(np.float64) - exact), fc.H2_MAX_REL_ERR * mag)
    yard = _fp32_mfma_ratio(p, inp)
    print('%s: worst error / (H2_MAX_REL_ERR * mag): split %.4f, fp32 MFMA %.4f' % (
        name, mine, yard))
    assert mine <= 1.5 * yard, (name, mine, yard)


# ------------------------------------------------------------------------------- routing ---
def _route_group(lib, name):
  entry = {r[0]: r for r in fc.ROUTES}[name]
  _, problems, has, expect = entry
  case = fc.Case(name, 'gemv' if expect == 'gemv' else 'split', problems, ['vec'])
  inputs = [fc.make_inputs(p, 'signed', 500 + i) for i, p in enumerate(problems)]
  return Group(lib, case, has=has, inputs=inputs), expect


def test_routing_m8_single_is_the_gemv_whatever_weights_come_along(lib):
  outs = {}
  for name in ('m8_wp', 'm8_wp_ws', 'm8_wp_wh_bound'):
    g, expect = _route_group(lib, name)
    assert expect == 'gemv' and fc.route(g.case.problems, set(g.problems[0].has)) == 'gemv'
    outs[name] = g.run()
    _check_writes(g.case, outs[name][0])
    _check_gemv(g, outs[name][0])
  _same(outs['m8_wp'], outs['m8_wp_ws'], 'Wp + Ws')
  _same(outs['m8_wp'], outs['m8_wp_wh_bound'], 'Wp + Wh + bound')
  g, expect = _route_group(lib, 'm8_relu_in')
  assert expect == 'gemv'
  res = g.run()
  _check_writes(g.case, res[0])
  _check_gemv(g, res[0])
  assert not np.array_equal(res[0][0], outs['m8_wp'][0][0])       # relu_in was applied


@pytest.mark.parametrize('name', [r[0] for r in fc.ROUTES if r[3] == 'refused'])
def test_routing_refusals_happen_before_any_launch(lib, name):
  g, _ = _route_group(lib, name)
  assert fc.route(g.case.problems, set(g.problems[0].has)) == 'refused'
  out = g.buffers()
  rcs, keep = g.call(out)
  torch.cuda.synchronize()
  assert rcs[0] < 0, name
  msg = lib.epos_last_error().decode('utf-8', 'replace')
  assert msg, name
  if name in fc.SMALL_M_REFUSALS:
    assert 'M <= 8' in msg and 'neither' not in msg, msg
  for b in out[0]:
    assert bool((b == fc.SENTINEL_BITS).all()), name
  for s in out[1]:
    assert s is None or not bool(s.any()), name
  del keep


def test_routing_m9_with_ws_is_the_split_kernel_and_agrees_with_the_gemv_rows(lib):
  """M = 9 with Ws and no Wh is computed by the split kernel within its bar; its first eight
  rows agree with the M = 8 GEMV of the same rows within the sum of the two kernels' bounds."""
  g9, expect = _route_group(lib, 'm9_ws')
  assert expect == 'split'
  res9 = g9.run()
  _check_writes(g9.case, res9[0])
  _check_split(g9, res9[0])
  p9, inp9 = g9.case.problems[0], g9.inputs[0]
  p8 = p9._replace(m=8)
  inp8 = fc.Inputs(inp9.a[:8], inp9.w, inp9.bias, None)
  g8 = Group(lib, fc.Case('m8_rows', 'gemv', [p8], ['m_8']), has=('Ws',), inputs=[inp8])
  res8 = g8.run()
  _check_writes(g8.case, res8[0])
  _check_gemv(g8, res8[0])
  _, mag = fc.expectation(p8, inp8)
  tol = fc.gemv_bound(p8, mag) + fc.H2_MAX_REL_ERR * mag
  err = np.abs(g9.values(res9[0], 0)[:8].astype(np.float64) - g8.values(res8[0], 0))
  print('M = 9 split rows against the M = 8 GEMV: worst difference / (sum of the bounds) = %.4f'
        % _ratio(err, tol))
  assert (err <= tol).all()


def test_gemv_row_of_eight_has_the_bytes_of_the_row_alone(lib):
  case = CASES[fc.ROW_ALONE_CASE]
  g = Group(lib, case)
  res = g.run()
  p, = case.problems
  inp = g.inputs[0]
  for m in range(p.m):
    one = fc.Case('row%d' % m, 'gemv', [p._replace(m=1)], ['m_1'])
    g1 = Group(lib, one, has=(), inputs=[fc.Inputs(inp.a[m:m + 1], inp.w, inp.bias,
                                                   inp.r[m:m + 1] if p.res else None)])
    r1 = g1.run()
    _check_writes(one, r1[0])
    assert np.array_equal(g1.values(r1[0], 0).view(np.uint32),
                          g.values(res[0], 0)[m:m + 1].view(np.uint32)), m


# ------------------------------------------------------------ history, stream and graph ---
@pytest.mark.parametrize('pair', fc.HISTORY_PAIRS, ids=lambda p: p[0])
def test_launch_is_independent_of_the_one_before(lib, pair):
  """X, then a different case Y (another kernel or another instantiation), then X again, back
  to back on the stream: each gives the bytes it gives alone."""
  gx, gy = (Group(lib, CASES[n]) for n in pair)
  x0, y0 = gx.run(), gy.run()
  _check_writes(gx.case, x0[0])
  _check_writes(gy.case, y0[0])
  ox, oy, ox2 = gx.buffers(), gy.buffers(), gx.buffers()
  keep = [gx.launch(ox), gy.launch(oy), gx.launch(ox2)]
  torch.cuda.synchronize()
  del keep
  _same(x0, Group.fetch(ox), 'X before Y')
  _same(y0, Group.fetch(oy), 'Y after X')
  _same(x0, Group.fetch(ox2), 'X after Y')


@pytest.mark.parametrize('name', fc.STREAM_CASES)
def test_on_a_non_default_stream(lib, name):
  g = Group(lib, CASES[name])
  ref = g.run()
  _check_writes(g.case, ref[0])
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  with torch.cuda.stream(s):
    assert torch.cuda.current_stream().cuda_stream == s.cuda_stream
    out = g.run()
  _same(ref, out, 'non-default stream')


@pytest.mark.parametrize('name', fc.GRAPH_CASES)
def test_in_a_captured_graph(lib, name):
  """One launch captured on a single stream (after an eager one: the first launch of a split
  instantiation sets its LDS attribute) and replayed twice into re-sentinelled buffers: the
  eager bytes."""
  g = Group(lib, CASES[name])
  eager = g.run()
  _check_writes(g.case, eager[0])
  out = g.buffers()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    keep = g.launch(out)
  for _ in range(2):
    for b in out[0]:
      b.fill_(fc.SENTINEL_BITS)
    graph.replay()
    torch.cuda.synchronize()
    _same(eager, Group.fetch(out), 'graph replay')
  del keep
