"""The fp16-pair GEMM on a PRE-SPLIT A operand (pointwise_gemm_h2_f32 with EposPointwiseArgs.
a_presplit, csrc/pointwise_gemm_h2.hip) in every launch regime of tests/helpers/
h2_presplit_cases.py, through the C ABI. A is written on the host as fp16 pairs -- canonical
splits and pair patterns no canonical split produces --, so the kernel is held against fp64 on
exactly the values the pairs stand for. Every case asserts
 (a) accuracy: |got - exact| <= H2_MAX_REL_ERR * mag elementwise, finite output (the 'inf' scale:
     the rows that hold a non-finite element come out non-finite, the others are held as usual);
 (b) no stray writes: C lies in a sentinel-filled buffer with guard rows before and behind, A's
     padding columns and the rows behind M - 1 are NaN in both fp16 halves;
 (c) the bytes of the fp32-A path on the same problem, slots, gain and bias (canonical kinds);
 (d) the same bytes with 128 x 128 and 128 x 64 tiles, as a group and problem by problem, and in
     two consecutive runs;
 (e) c_amax == max |C| exactly, also for a group writing column slices of one buffer;
 (f) col_sums within 31 * 2^-24 * sum |c| of the fp64 block sums of the stored C, C unchanged by
     the extra output, the pooled means, the sentinels around the block sums.
The inputs and fp64 expectations are computed once per problem (helpers' lru_cache)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import h2_presplit_cases as pc
from helpers import pointwise_wgrad_ref as wr

pytestmark = pytest.mark.gpu

CASES = pc.by_name(pc.CASES)
SENT = np.int32(pc.SENTINEL_BITS)


@pytest.fixture(scope='module')
def lib():
  from epos_amd import _lib
  assert torch.cuda.is_available(), 'GPU tests need a HIP device'
  return _lib.load()


@pytest.fixture(autouse=True)
def tile_limit(lib):
  """The tests set epos_set_h2_narrow_tile_limit per launch; the process's value comes back."""
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
  return torch.full(shape, pc.SENTINEL_BITS, dtype=torch.int32, device='cuda')


def _pack(lib, w, which):
  k, n = w.shape
  fn = {'plain': lib.epos_pack_pointwise_weights,
        'h2': lib.epos_pack_pointwise_weights_h2}[which]
  w = np.ascontiguousarray(w, np.float32)
  src = w.ctypes.data_as(ctypes.c_void_p)
  total = fn(src, k, n, None)
  assert total > 0, which
  dst = np.empty(total, np.float32 if which == 'plain' else np.uint8)
  fn(src, k, n, dst.ctypes.data_as(ctypes.c_void_p))
  return torch.from_numpy(dst).cuda()


def _slot(word=None, at=0):
  from epos_amd import _lib
  s = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device='cuda')
  if word is not None:
    s[at] = int(np.array([word], np.uint32).view(np.int32)[0])
  return s


def _slot_value(slot):
  return float(slot.cpu().numpy().view(np.float32).max())


class Problem(object):
  """One problem's inputs on the device."""

  def __init__(self, lib, case, i):
    self.p = p = case.problems[i]
    inp = pc.inputs(case.name, i)
    self.A = {1: _dev(pc.a_buffer(case, i, True))}
    if case.values in pc.CANONICAL:
      self.A[0] = _dev(pc.a_buffer(case, i, False))
    assert all(a.data_ptr() % 16 == 0 for a in self.A.values())
    self.slot = _slot(inp.slot, 37)               # one word: the bound is the maximum of all 64
    self.slot2 = _slot(inp.slot2, 5) if inp.slot2 is not None else None
    self.gain, self.bias_a = inp.gain, inp.bias_a
    self.Wp, self.Wh = _pack(lib, inp.w, 'plain'), _pack(lib, inp.w, 'h2')
    self.bias = self.R = None
    if p.bias:                                    # padded to 128 floats; NaN behind the N values
      b = np.full(-(-p.n // 128) * 128, np.nan, np.float32)
      b[:p.n] = inp.bias
      self.bias = _dev(b)
    if p.res:
      r = np.full((p.m, p.ldr), np.nan, np.float32)
      r[:, :p.n] = inp.r
      self.R = _dev(r)


class Group(object):
  """A case's inputs on the device, its launches and their outputs on the host."""

  def __init__(self, lib, case):
    self.lib, self.case = lib, case
    self.problems = [Problem(lib, case, i) for i in range(len(case.problems))]
    self.layout, self.places = pc.layout(case), pc.places(case)

  def buffers(self):
    """Fresh outputs: (C buffers, c_amax slots per problem, col_sums buffers per problem)."""
    bufs = [_sentinels(b.floats) for b in self.layout]
    assert all(b.data_ptr() % 512 == 0 for b in bufs)
    shared_slot = _slot() if self.case.shared else None
    amax = [(shared_slot if self.case.shared else _slot()) if d.p.c_amax else None
            for d in self.problems]
    sums = [_sentinels(pc.sums_rows(d.p), d.p.n + 4) if d.p.col_sums else None
            for d in self.problems]
    return bufs, amax, sums

  def args(self, out, presplit=1, col_sums=True):
    from epos_amd import _lib
    bufs, amax, sums = out
    arr = (_lib.PointwiseArgs * len(self.problems))()
    for i, (d, (bi, off, ldc)) in enumerate(zip(self.problems, self.places)):
      p = d.p
      arr[i] = _lib.PointwiseArgs(
          A=d.A[presplit].data_ptr(), lda=p.lda, Wp=d.Wp.data_ptr(),
          bias=d.bias.data_ptr() if d.bias is not None else None,
          R=d.R.data_ptr() if d.R is not None else None, ldr=p.ldr,
          C=bufs[bi].data_ptr() + 4 * off, ldc=ldc, M=p.m, N=p.n, K=p.k, relu=p.relu, relu_in=0,
          sub=1, Wh=d.Wh.data_ptr(), a_amax=d.slot.data_ptr(),
          a_amax2=d.slot2.data_ptr() if d.slot2 is not None else None, a_gain=d.gain,
          a_bias=d.bias_a, a_presplit=presplit,
          c_amax=amax[i].data_ptr() if amax[i] is not None else None,
          col_sums=sums[i].data_ptr() if col_sums and sums[i] is not None else None,
          col_ld=p.n + 4 if p.col_sums else 0, c_stream=p.c_stream)
    return arr

  def launch(self, out, limit=None, presplit=1, col_sums=True, one_by_one=False):
    """Enqueues the case on the current stream; returns what must stay alive."""
    from epos_amd import _lib
    self.lib.epos_set_h2_narrow_tile_limit(self.case.limit if limit is None else limit)
    arr = self.args(out, presplit, col_sums)
    if one_by_one:
      for i in range(len(self.problems)):
        _lib.check(self.lib.epos_pointwise_conv_f32(ctypes.byref(arr[i]), _stream()), 'single')
    else:
      _lib.check(self.lib.epos_pointwise_conv_grouped_f32(arr, len(self.problems), _stream()),
                 self.case.name)
    return arr

  @staticmethod
  def fetch(out):
    bufs, amax, sums = out
    return ([b.cpu().numpy() for b in bufs],
            [_slot_value(a) if a is not None else None for a in amax],
            [s.cpu().numpy() if s is not None else None for s in sums])

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
  """Equal bytes of two fetched results (C buffers, c_amax values, block sums)."""
  for x, y in zip(a[0], b[0]):
    diff = np.flatnonzero(x != y)
    assert diff.size == 0, '%s: %d words of C differ (first at %d)' % (what, diff.size, diff[0])
  assert a[1] == b[1], (what, a[1], b[1])
  for x, y in zip(a[2], b[2]):
    assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), what


def _check_writes(case, bufs):
  """(b): everything the case must write is written, every other word keeps the sentinel."""
  for bi, out in enumerate(bufs):
    mask = pc.written_mask(case, bi)
    left = int((out[mask] == SENT).sum())
    assert left == 0, '%s: %d elements of buffer %d unwritten' % (case.name, left, bi)
    broken = np.flatnonzero(out[~mask] != SENT)
    assert broken.size == 0, '%s: %d words written outside [M) x [c_off, c_off + N) of buffer ' \
        '%d (first at index %d of the outside)' % (case.name, broken.size, bi, broken[0])


def _check_fp64(g, bufs):
  """(a); returns the worst error / bound."""
  case, worst = g.case, 0.0
  for i, p in enumerate(case.problems):
    exact, mag = pc.expected(case.name, i)
    bad = pc.inputs(case.name, i).bad_rows
    got = g.values(bufs, i)
    if case.scale == 'inf':
      assert bad.sum() == 2
      assert not np.isfinite(got[bad]).any(), '%s: a row fed by a non-finite element came out ' \
          'finite' % case.name
    assert np.isfinite(got[~bad]).all(), '%s: problem %d has non-finite values' % (case.name, i)
    err = np.abs(got[~bad].astype(np.float64) - exact[~bad])
    bound = pc.H2_MAX_REL_ERR * mag[~bad]
    ratio = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max())
    worst = max(worst, ratio)
    print('%s problem %d (%d x %d x %d): worst error / (H2_MAX_REL_ERR * mag) = %.4f' % (
        case.name, i, p.m, p.n, p.k, ratio))
    assert (err <= bound).all(), (case.name, i, ratio)
  return worst


def _check_amax(g, res):
  """(e): the slot holds max |C| over what the launch wrote -- a shared slot over every slice."""
  case = g.case
  bufs, amax, _ = res
  tops = [float(np.abs(g.values(bufs, i)).max()) for i in range(len(case.problems))]
  for i, p in enumerate(case.problems):
    if p.c_amax:
      want = max(t for t, q in zip(tops, case.problems) if q.c_amax) if case.shared else tops[i]
      assert amax[i] == want, (case.name, i, amax[i], want)
      assert want > 0


def _check_sums(g, res):
  """(f); returns the worst error / bound."""
  case, worst = g.case, 0.0
  bufs, _, sums = res
  for i, p in enumerate(case.problems):
    if not p.col_sums:
      continue
    c = g.values(bufs, i).astype(np.float64)
    blocks = -(-p.m // 32)
    got = sums[i][:blocks, :p.n].view(np.float32).astype(np.float64)
    outside = np.ones(sums[i].shape, bool)
    outside[:blocks, :p.n] = False
    assert (sums[i][outside] == SENT).all(), '%s: block sums written past ceil(M/32) rows or ' \
        'N columns' % case.name
    for b in range(blocks):
      rows = c[32 * b:min(32 * b + 32, p.m)]          # the partial last block: its live rows
      ref, tol = rows.sum(0), 31 * 2.0 ** -24 * np.abs(rows).sum(0)
      err = np.abs(got[b] - ref)
      ratio = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
      worst = max(worst, ratio)
      assert (err <= tol).all(), (case.name, b, ratio)
    print('%s: worst block-sum error / (31 * 2^-24 * sum |c|) = %.4f' % (case.name, worst))
  return worst


def _check_means(g, res):
  """The image-pooling means (epos_global_avg_pool_partial_f32 over the block sums) against the
  fp64 mean of the stored C: the block sums' bound, the (blocks - 1) further additions and the
  division, each within 2^-24 -- (31 + blocks) * 2^-24 * mean |c|."""
  from epos_amd import _lib
  case = g.case
  bufs, _, sums = res
  for i, p in enumerate(case.problems):
    if not (p.col_sums and p.images > 1):
      continue
    hw = p.m // p.images
    blocks = hw // 32
    part = _dev(sums[i])
    y = _sentinels(p.images + 1, p.n)
    _lib.check(g.lib.epos_global_avg_pool_partial_f32(part.data_ptr(), p.n + 4, y.data_ptr(),
                                                      p.images, blocks, p.n, hw, _stream()))
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert (y[p.images:] == SENT).all()
    c = g.values(bufs, i).astype(np.float64).reshape(p.images, hw, p.n)
    got = y[:p.images].view(np.float32).astype(np.float64)
    tol = (31 + blocks) * 2.0 ** -24 * np.abs(c).mean(1)
    assert (np.abs(got - c.mean(1)) <= tol).all(), case.name


def _finite_rows_equal(g, a, b, what):
  """(c) for the 'inf' scale: the same finite / non-finite pattern, equal bytes wherever finite
  (the payload of a NaN that a host-made NaN half went into is not part of the contract)."""
  for i in range(len(g.case.problems)):
    x, y = g.values(a[0], i), g.values(b[0], i)
    fin = np.isfinite(x)
    assert np.array_equal(fin, np.isfinite(y)), what
    assert np.array_equal(x[fin].view(np.uint32), y[fin].view(np.uint32)), what


@pytest.mark.parametrize('name', [c.name for c in pc.CASES])
def test_presplit_regime(lib, name):
  case = CASES[name]
  g = Group(lib, case)
  res = g.run()
  _check_writes(case, res[0])
  worst = _check_fp64(g, res[0])
  _check_amax(g, res)
  worst_sums = _check_sums(g, res)
  _check_means(g, res)
  print('%s: worst error / bound: fp64 %.4f, col_sums %.4f' % (name, worst, worst_sums))
  # (d) two consecutive runs, the other tile width, problem by problem
  _same(res, g.run(), name + ': second run')
  other = g.run(limit=0 if case.limit else pc.BIG)
  _same(res, other, name + ': other tile limit')
  _check_writes(case, other[0])
  if len(case.problems) > 1:
    for limit in (0, pc.BIG):
      _same(res, g.run(limit=limit, one_by_one=True), name + ': problem by problem')
  # (c) the fp32-A path splits the same values with the same slots into the same pairs
  if case.values in pc.CANONICAL:
    f32 = g.run(presplit=0)
    _check_writes(case, f32[0])
    if case.scale == 'inf':
      _finite_rows_equal(g, res, f32, name + ': fp32 A')
    else:
      _same(res, f32, name + ': fp32 A')
  # (f) C is the same with and without the block sums
  if any(p.col_sums for p in case.problems):
    plain = g.run(col_sums=False)
    for x, y in zip(res[0], plain[0]):
      assert np.array_equal(x, y), name + ': C changed by col_sums'
    assert all((s == SENT).all() for s in plain[2] if s is not None)


@pytest.mark.parametrize('limit', [0, pc.BIG])
def test_presplit_c_amax_sees_every_wave_and_column_block(lib, limit):
  """The maximum of |C| planted in turn into each wave's rows of both row tiles and each column
  block of both column tiles (one row of A at the bound, the others a hundredth of it, W >= 0,
  one large bias): the slot holds exactly that element every time -- a reduction that lost one
  wave, half-wave or column block would only show when the maximum happens to sit there."""
  from epos_amd import _lib
  m, n, k = 137, 200, 48
  rng = np.random.default_rng(3)
  base = np.maximum(rng.standard_normal((m, k)), 0).astype(np.float32) * np.float32(0.01)
  w = np.abs(rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)
  Wp, Wh = _pack(lib, w, 'plain'), _pack(lib, w, 'h2')
  top = np.float32(4.0)
  slot = _slot(int(top.view(np.uint32)), 11)
  s, _ = wr.h2_scale(top)
  lib.epos_set_h2_narrow_tile_limit(limit)
  for r, c in ((0, 5), (37, 40), (70, 70), (100, 100), (127, 130), (128, 165), (136, 199)):
    x = base.copy()
    x[r] = rng.uniform(2, 4, k).astype(np.float32)
    bias = np.zeros(256, np.float32)
    bias[c] = 50
    A, Bd = _dev(pc.encode(x, s)), _dev(bias)
    C, cs = _sentinels(m, n), _slot()
    args = _lib.PointwiseArgs(A=A.data_ptr(), lda=k, Wp=Wp.data_ptr(), bias=Bd.data_ptr(), R=None,
                              ldr=0, C=C.data_ptr(), ldc=n, M=m, N=n, K=k, relu=0, relu_in=0,
                              sub=1, Wh=Wh.data_ptr(), a_amax=slot.data_ptr(), a_presplit=1,
                              c_amax=cs.data_ptr())
    _lib.check(lib.epos_pointwise_conv_f32(ctypes.byref(args), _stream()))
    torch.cuda.synchronize()
    got = C.cpu().numpy().view(np.float32)
    assert np.isfinite(got).all()
    assert np.unravel_index(np.abs(got).argmax(), got.shape) == (r, c)
    assert _slot_value(cs) == float(np.abs(got).max()), (r, c)


# ----------------------------------------------------------------------------- refusals ---
@pytest.mark.parametrize('what', pc.REFUSALS)
def test_presplit_refusals(lib, what):
  """Each of these is refused by the entry point before anything is launched: the return value
  is an error and every output keeps its sentinels."""
  from epos_amd import _lib
  case = CASES[pc.REFUSAL_CASE]
  g = Group(lib, case)
  p = case.problems[0]
  bufs, _, _ = out = g.buffers()
  one = g.args(out)[0]
  extra = []
  count = 1
  arr = (_lib.PointwiseArgs * 2)(one, one)
  if what == 'no_a_amax':
    arr[0].a_amax = None
  elif what == 'sub_2':
    arr[0].sub, arr[0].Ho, arr[0].Wo, arr[0].Hi, arr[0].Wi = 2, 1, p.m, 1, p.m
  elif what == 'relu_in':
    arr[0].relu_in = 1
  elif what == 'm_8':
    arr[0].M = 8
  elif what == 'mixed_kinds':
    c2 = _sentinels(pc.layout(case)[0].floats)
    extra.append(c2)
    arr[1].C = c2.data_ptr() + 4 * g.places[0][1]
    arr[1].A, arr[1].a_presplit = g.problems[0].A[0].data_ptr(), 0
    count = 2
  else:                                   # 'col_sums_with_residual'
    r = _sentinels(p.m, p.n)
    sums = _sentinels(pc.sums_rows(p), p.n + 4)
    extra += [r, sums]
    arr[0].R, arr[0].ldr = r.data_ptr(), p.n
    arr[0].col_sums, arr[0].col_ld = sums.data_ptr(), p.n + 4
  for limit in (0, pc.BIG):
    lib.epos_set_h2_narrow_tile_limit(limit)
    rc = lib.epos_pointwise_conv_grouped_f32(arr, count, _stream())
    assert rc != 0 and lib.epos_last_error(), what
  torch.cuda.synchronize()
  for t in bufs + extra:
    assert bool((t == pc.SENTINEL_BITS).all()), what
  # ... and the same arguments without the fault run
  res = g.run()
  _check_writes(case, res[0])


# -------------------------------------------------- producer and consumer on padded rows ---
def test_depthwise_pairs_on_padded_rows_feed_the_presplit_gemm(lib):
  """The plan's pairing at a small size: the depthwise kernel writes C = 40 channels as fp16
  pairs into rows of pitch 64 (the plan rounds the pitch up to 32 floats), the pre-split GEMM
  reads them with lda = 64. The padding columns keep their sentinel through both launches, the
  GEMM is within H2_MAX_REL_ERR * mag of fp64 on the decoded intermediate, and its output has
  the bytes of the ldy = lda = 40 run."""
  from epos_amd import _lib
  rng = np.random.default_rng(11)
  b, h, w, c, n, rate = 2, 9, 11, 40, 136, 3
  m = b * h * w
  x = rng.standard_normal((b, h, w, c)).astype(np.float32)
  w9c = (rng.standard_normal((9, c)) * 0.4).astype(np.float32)
  dbias = rng.standard_normal(c).astype(np.float32)
  wk = (rng.standard_normal((c, n)) / np.sqrt(c)).astype(np.float32)
  X, W9, Bd = _dev(x), _dev(w9c), _dev(dbias)
  Wp, Wh = _pack(lib, wk, 'plain'), _pack(lib, wk, 'h2')
  xs = _slot()
  _lib.check(lib.epos_absmax_f32(X.data_ptr(), c, m, c, xs.data_ptr(), _stream()))
  gain = float(np.abs(w9c.astype(np.float64)).sum(0).max())
  bias0 = float(np.abs(dbias).max())
  outs = {}
  for ld in (64, 40):
    T = _sentinels(m + 4, ld)                       # four sentinel rows behind the last pixel
    C = _sentinels(pc.GUARD_BEFORE + m + pc.guard_after(m), n)
    dw = _lib.DepthwiseArgs(X=X.data_ptr(), ldx=c, w9c=W9.data_ptr(), bias=Bd.data_ptr(),
                            Y=T.data_ptr(), ldy=ld, B=b, Hi=h, Wi=w, Ho=h, Wo=w, C=c, stride=1,
                            rate=rate, relu_in=0, relu_out=1, y_h2=1, x_amax=xs.data_ptr(),
                            gain=gain, bias0=bias0)
    pw = _lib.PointwiseArgs(A=T.data_ptr(), lda=ld, Wp=Wp.data_ptr(), bias=None, R=None, ldr=0,
                            C=C.data_ptr() + 4 * pc.GUARD_BEFORE * n, ldc=n, M=m, N=n, K=c, relu=0,
                            relu_in=0, sub=1, Wh=Wh.data_ptr(), a_amax=xs.data_ptr(), a_gain=gain,
                            a_bias=bias0, a_presplit=1)
    _lib.check(lib.epos_depthwise3x3_f32(ctypes.byref(dw), _stream()), 'depthwise')
    _lib.check(lib.epos_pointwise_conv_f32(ctypes.byref(pw), _stream()), 'pointwise')
    torch.cuda.synchronize()
    outs[ld] = (T.cpu().numpy(), C.cpu().numpy())
  t64, c64 = outs[64]
  t40, c40 = outs[40]
  assert (t64[:m, c:] == SENT).all() and (t64[m:] == SENT).all() and (t40[m:] == SENT).all()
  assert not (t64[:m, :c] == SENT).any() and np.array_equal(t64[:m, :c], t40[:m])
  rows = slice(pc.GUARD_BEFORE, pc.GUARD_BEFORE + m)
  assert (c64[:rows.start] == SENT).all() and (c64[rows.stop:] == SENT).all()
  assert np.array_equal(c64, c40)
  bound = wr.slot_bound(xs.cpu().numpy().view(np.uint32), None, gain, bias0)
  assert np.float32(np.float32(gain) * np.abs(x).max()) + np.float32(bias0) == bound
  _, inv = wr.h2_scale(bound)
  a64 = wr.h2_values(t64[:m].view(np.uint32), c, inv)
  assert np.isfinite(a64).all() and a64.min() >= 0 and a64.max() > 0          # relu_out
  got = c64[rows].view(np.float32)
  exact = a64 @ wk.astype(np.float64)
  mag = np.abs(a64) @ np.abs(wk).astype(np.float64)
  ratio = float((np.abs(got - exact) / (pc.H2_MAX_REL_ERR * mag)).max())
  print('depthwise pairs -> presplit GEMM: worst error / (H2_MAX_REL_ERR * mag) = %.4f' % ratio)
  assert np.isfinite(got).all() and ratio <= 1.0


# ------------------------------------------------------------ history, stream and graph ---
def test_presplit_launch_is_independent_of_the_one_before(lib):
  """X, then a different case Y (other instantiation, tile width, K-step count, epilogue), then
  X again, back to back on the stream: each gives the bytes it gives alone."""
  gx, gy = (Group(lib, CASES[n]) for n in pc.HISTORY_PAIR)
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


def test_presplit_on_a_non_default_stream(lib):
  g = Group(lib, CASES[pc.STREAM_CASE])
  ref = g.run()
  _check_writes(g.case, ref[0])
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  with torch.cuda.stream(s):
    assert torch.cuda.current_stream().cuda_stream == s.cuda_stream
    out = g.run()
  _same(ref, out, 'non-default stream')


def test_presplit_in_a_captured_graph(lib):
  """One launch captured on a single stream (after an eager one: the first fp16-pair launch on
  a device allocates) and replayed twice into re-sentinelled buffers: the eager bytes."""
  g = Group(lib, CASES[pc.GRAPH_CASE])
  eager = g.run()
  _check_writes(g.case, eager[0])
  out = g.buffers()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    keep = g.launch(out)
  for _ in range(2):
    for b in out[0]:
      b.fill_(pc.SENTINEL_BITS)
    graph.replay()
    torch.cuda.synchronize()
    _same(eager, Group.fetch(out), 'graph replay')
  del keep
